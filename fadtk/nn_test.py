from fadtk_amd.nn_test import *          # noqa: F401,F403
from fadtk_amd.nn_test import NearestNeighbourTest, calc_nearest_neighbour_test, main   # noqa: F401

if __name__ == "__main__":
    main()
