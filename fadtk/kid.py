from fadtk_amd.kid import *          # noqa: F401,F403
from fadtk_amd.kid import KernelDistance, calc_kernel_distance, calc_kernel_distance_full, main   # noqa: F401

if __name__ == "__main__":
    main()
