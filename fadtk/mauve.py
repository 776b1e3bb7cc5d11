from fadtk_amd.mauve import *           # noqa: F401,F403
from fadtk_amd.mauve import (CELLS_CSV_HEADER, CSV_HEADER, Mauve, calc_kmeans, calc_mauve, histogram_metrics, main,   # noqa: F401
                             seed_rows)

if __name__ == "__main__":
    main()
