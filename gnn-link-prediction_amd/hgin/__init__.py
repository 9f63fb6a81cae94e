"""hgin — MI355X-native (gfx950) heterogeneous-GIN training hot path.

Drop-in for the reference's ``models.py`` surface (HetroGIN / GINLayer / GINConv over a PyG-style
HeteroConv / MessagePassing), with the message + aggregate, the self term, the MLP update (MFMA), their
backward, the CSR build, the negative sampler and the link decoder in hand-written HIP (libhgin.so, C ABI
in include/hgin.h).  See DESIGN.md.
"""
from . import data  # noqa: F401
from ._lib import HginError, HginUnavailable, build  # noqa: F401
from .conv import GINConv, GINLayer, HeteroConv, MessagePassing, reset  # noqa: F401
from .linkpred import (LINK_OBJECTIVES, LinkBatch, LinkPredictor, LinkSegments, hard_negatives, hard_negatives_seg, link_full_metrics, link_full_ranks,  # noqa: F401
                       link_metrics, link_neighbor_batch, link_neighbor_batch_excl, link_ranks, link_topk, sampled_link_loss)
from .linkpred import full_softmax_link_loss, link_lse, link_lse_unfused  # noqa: F401
from .linksplit import LinkSplit, link_split, link_split_parts, link_split_select  # noqa: F401
from .models import HetroGAT, HetroGIN  # noqa: F401
from .neighbor import NeighborSampler, SampledSubgraph  # noqa: F401
from .qt import QTBaseline  # noqa: F401
from .train import link_minibatch_step, link_train_step  # noqa: F401

__all__ = ["HetroGIN", "HetroGAT", "QTBaseline", "GINLayer", "GINConv", "HeteroConv", "MessagePassing", "reset", "build",
           "HginError", "HginUnavailable", "data", "LinkPredictor", "sampled_link_loss", "link_ranks", "link_metrics",
           "link_full_ranks", "link_full_metrics", "link_topk", "link_train_step", "LINK_OBJECTIVES", "hard_negatives",
           "LinkSegments", "hard_negatives_seg", "LinkSplit", "link_split", "link_split_parts", "link_split_select",
           "NeighborSampler", "SampledSubgraph", "LinkBatch", "link_neighbor_batch", "link_minibatch_step", "link_lse",
           "link_lse_unfused", "full_softmax_link_loss", "link_neighbor_batch_excl"]
