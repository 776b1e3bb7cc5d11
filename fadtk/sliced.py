from fadtk_amd.sliced import *          # noqa: F401,F403
from fadtk_amd.sliced import SlicedWasserstein, calc_sliced_wasserstein, main   # noqa: F401

if __name__ == "__main__":
    main()
