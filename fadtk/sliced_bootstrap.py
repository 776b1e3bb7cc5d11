from fadtk_amd.sliced_bootstrap import *          # noqa: F401,F403
from fadtk_amd.sliced_bootstrap import CSV_HEADER, PAIR_KIND, SET_KIND, main   # noqa: F401
