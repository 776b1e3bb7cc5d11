"""fadtk_amd -- MI355X-native Frechet Audio Distance engine behind fadtk's plugin surface.

The FAD hot path (running mean/covariance of embedding frames, matrix square root of
Sigma1 Sigma2, batched per-song scores, log-mel front ends) runs in hand-written HIP for gfx950
(`fadtk_amd/csrc`, C ABI in `include/fad_hip.h`).  This package is the host-side mirror of
fadtk's public interface over that library.
"""
from .fad import FADInfResults, FrechetAudioDistance, calc_embd_statistics, calc_frechet_distance  # noqa: F401
from .utils import (PathLike, calculate_embd_statistics_online, dataset_statistics, find_sox_formats,  # noqa: F401
                    get_cache_embedding_path)

__version__ = "0.1.0"


def __getattr__(name):
    # loaders and the batch driver import torch; keep `import fadtk_amd` light
    if name in ("ModelLoader", "get_all_models", "VGGishModel", "EncodecEmbModel", "CLAPLaionModel", "WhisperModel",
                "W2V2Model", "HuBERTModel", "WavLMModel", "MERTModel"):
        from . import model_loader
        return getattr(model_loader, name)
    if name in ("KernelAudioDistance", "calc_kernel_audio_distance", "calc_kernel_audio_distance_individual",
                "calc_kernel_audio_distance_uncertainty", "KadUncertainty",
                "calc_kernel_audio_distance_permutation_test", "calc_kernel_audio_distance_sweep", "KadSweep",
                "calc_kernel_audio_distance_aggregated_test",
                "KAD_KERNELS"):      # lazy: `python -m fadtk_amd.kad` runs the module itself
        from . import kad
        return getattr(kad, name)
    if name in ("PrecisionRecall", "calc_precision_recall_density_coverage"):      # lazy, as KAD's
        from . import prdc
        return getattr(prdc, name)
    if name in ("NearestNeighbours", "calc_nearest_neighbours", "calc_authenticity"):      # lazy, as KAD's
        from . import nearest
        return getattr(nearest, name)
    if name in ("NearestNeighbourTest", "calc_nearest_neighbour_test"):      # lazy, as KAD's
        from . import nn_test
        return getattr(nn_test, name)
    if name in ("KernelDistance", "calc_kernel_distance", "calc_kernel_distance_full"):      # lazy, as KAD's
        from . import kid
        return getattr(kid, name)
    if name in ("SinkhornDivergence", "calc_sinkhorn_divergence"):      # lazy, as KAD's
        from . import sinkhorn
        return getattr(sinkhorn, name)
    if name in ("SlicedWasserstein", "calc_sliced_wasserstein", "calc_sliced_wasserstein_individual", "calc_sliced_wasserstein_shares",
                "calc_sliced_wasserstein_permutation_test", "calc_sliced_wasserstein_bootstrap",
                "calc_sliced_wasserstein_bootstrap_compare", "bootstrap_counts", "sliced_directions"):      # lazy, as KAD's
        from . import sliced
        return getattr(sliced, name)
    if name in ("Mauve", "calc_mauve", "calc_kmeans"):      # lazy, as KAD's
        from . import mauve
        return getattr(mauve, name)
    if name == "cache_embedding_files":
        from .fad_batch import cache_embedding_files
        return cache_embedding_files
    raise AttributeError(name)
