from fadtk_amd.sinkhorn import *          # noqa: F401,F403
from fadtk_amd.sinkhorn import SinkhornDivergence, calc_sinkhorn_divergence, main   # noqa: F401

if __name__ == "__main__":
    main()
