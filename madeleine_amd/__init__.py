"""madeleine_amd -- MI355X-native (gfx950) implementation of MADELEINE's cross-stain SSL pretrain hot path.

Drop-in surface (same names / signatures as the reference's madeleine.models.Model, madeleine.models.abmil,
madeleine.utils.loss, madeleine.utils.trainer):

    from madeleine_amd import MADELEINE, ABMILEmbedder, BatchedABMIL, create_model
    from madeleine_amd import InfoNCE, GOT, calculate_losses, train_loop, run_inference
    from madeleine_amd import AdamW          # torch.optim.AdamW's update with a device-side non-finite guard and clipping
    from madeleine_amd import DeviceSlideStore   # the cohort's features resident on the device, batches drawn by one kernel
    from madeleine_amd import linear_probe       # the few-shot linear-probing protocol, every (task, k, fold) fit in one batch of launches
    from madeleine_amd import linear_probe_cv    # the probe trained on all labels: stratified K folds, primal Newton-CG fits of any size
    from madeleine_amd import device_smooth_rank # the model-selection criterion (smooth rank of the embeddings) without a host SVD
    from madeleine_amd import cross_stain_retrieval  # at which rank a case's own IHC slide comes back for its H&E slide, and the reverse
    from madeleine_amd import survival_probe     # do the embeddings stratify patients: cross-validated Cox fits, C-index, log-rank
    from madeleine_amd import heatmap            # attention heatmaps on the device: render, gaussian_taps, colormap, save_png
    from madeleine_amd import linear_probe_ci    # bootstrap intervals of the probes' metrics and paired differences between encoders
    from madeleine_amd import attn_contrib, contrib_stats   # which patches made a probe's decision (DeviceSlideStore.contributions)
    from madeleine_amd import regression_probe   # continuous targets: batched ridge fits, Pearson, Spearman, R^2 on held-out cases

The numeric work runs in csrc/libmadeleine_amd.so through the C ABI of include/madeleine_amd.h (the heatmap renderer: of
include/madeleine_amd_view.h; the bootstrap counts: of include/madeleine_amd_stats.h; the patch contributions: of
include/madeleine_amd_explain.h; the regression probe: of include/madeleine_amd_regress.h).
Importing this package does not load the library (so model construction / state_dict handling works on
any box); the first forward does, and raises if it is unavailable -- there is no fallback path.
"""
from .abmil import BatchedABMIL
from .functional import attn_contrib, contrib_stats
from .loss import GOT, InfoNCE, info_nce, init_intra_wsi_loss_function
from .model import ABMILEmbedder, MADELEINE, create_model
from .optim import AdamW
from .retrieval import cross_stain_retrieval, retrieval_metrics, slide_neighbours
from .store import DeviceSlideStore, PackedBags
from .survival import fit_cox, survival_probe, survival_splits
from .trainer import calculate_losses, train_loop
from .utils import create_model_from_pretrained, device_smooth_rank, extract_slide_level_embeddings, load_checkpoint, run_inference

__all__ = ["MADELEINE", "ABMILEmbedder", "BatchedABMIL", "create_model", "InfoNCE", "info_nce", "GOT",
           "init_intra_wsi_loss_function", "calculate_losses", "train_loop", "run_inference", "extract_slide_level_embeddings",
           "load_checkpoint", "create_model_from_pretrained", "AdamW", "DeviceSlideStore", "PackedBags", "probe_splits", "fit_logistic",
           "linear_probe", "device_smooth_rank", "cross_stain_retrieval", "retrieval_metrics", "slide_neighbours",
           "survival_splits", "fit_cox", "survival_probe", "cv_splits", "linear_probe_cv", "heatmap", "render_heatmaps", "gaussian_taps",
           "colormap", "save_png", "bootstrap_summary", "paired_difference", "linear_probe_ci", "survival_probe_ci", "attn_contrib",
           "contrib_stats", "regression_splits", "fit_ridge", "regression_probe", "fit_kmeans", "assign_kmeans"]
__version__ = "0.2"
_HEATMAP = ("render_heatmaps", "gaussian_taps", "colormap", "save_png")
_PROBE = ("probe_splits", "fit_logistic", "linear_probe", "cv_splits", "linear_probe_cv")
_RESAMPLE = ("bootstrap_summary", "paired_difference", "linear_probe_ci", "survival_probe_ci")
_REGRESS = ("regression_splits", "fit_ridge", "regression_probe")
_CLUSTER = ("fit_kmeans", "assign_kmeans", "KMeansResult")


def __getattr__(name):
    """The linear probe's names resolve on first use, so that `python -m madeleine_amd.probe` runs a module nobody imported before."""
    if name in _PROBE:
        from . import probe
        return getattr(probe, name)
    if name in _RESAMPLE:      # imports the probe (above) and binds the third header's #defines: resolved on first use as well
        from . import resample
        return getattr(resample, name)
    if name in _REGRESS:       # binds the fifth header's #defines: resolved on first use as well
        from . import regress
        return getattr(regress, name)
    if name in _CLUSTER:       # binds the sixth header's #defines: resolved on first use as well
        from . import cluster
        return getattr(cluster, name)
    if name == "heatmap" or name in _HEATMAP:      # the renderer binds the library's #defines: resolved on first use as well
        import importlib
        mod = importlib.import_module(".heatmap", __name__)
        return mod if name == "heatmap" else getattr(mod, "render" if name == "render_heatmaps" else name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
