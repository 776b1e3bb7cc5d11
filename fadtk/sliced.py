from fadtk_amd.sliced import *          # noqa: F401,F403
from fadtk_amd.sliced import (INDIV_CSV_HEADER, SlicedWasserstein, calc_sliced_wasserstein,   # noqa: F401
                              calc_sliced_wasserstein_individual, calc_sliced_wasserstein_permutation_test,
                              calc_sliced_wasserstein_shares, main)

if __name__ == "__main__":
    main()
