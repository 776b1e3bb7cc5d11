from fadtk_amd.sliced_permutation import *          # noqa: F401,F403
from fadtk_amd.sliced_permutation import CSV_HEADER, main   # noqa: F401

if __name__ == "__main__":
    main()
