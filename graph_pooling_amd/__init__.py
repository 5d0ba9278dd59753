"""graph_pooling_amd — MI355X-native DiffPool forward/backward behind the reference's nn.Module surface.

    from graph_pooling_amd.encoders import SoftPoolingGcnEncoder, GcnEncoderGraph, GcnSet2SetEncoder
    from graph_pooling_amd.set2set import Set2Set
    from graph_pooling_amd import SparseGcnSet2SetEncoder      # GCN + Set2Set on CSR graphs and ragged batches (sparse.py)
    from graph_pooling_amd import EdgeAttention                # learned edge weights in front of the CSR encoders
    from graph_pooling_amd import GatConv                      # multi-head graph-attention layer on CSR graphs / batches
    from graph_pooling_amd import SageConv, SageEncoder        # GraphSAGE layer, the neighbour sample drawn on the device
    from graph_pooling_amd import NestedSageEncoder            # a SageConv stack on nested mini-batches (sampled blocks)
    from graph_pooling_amd import TopKPooling                  # hard top-k (gPool / SAGPool) pooling, the induced CSR on the device

The arithmetic lives in libdiffpool_hip.so (graph_pooling_amd/csrc, C ABI in include/diffpool_hip.h).
Importing this package does not load the library; the first forward does, and raises if it is missing.
"""
__version__ = "0.1.0"

__all__ = ["SparseGcnSet2SetEncoder", "EdgeAttention", "GatConv", "SageConv", "SageEncoder", "TopKPooling", "NestedSageEncoder"]


def __getattr__(name):
    # resolved on first use: importing the package (or graph_pooling_amd.ops alone) pulls in no model module
    if name == "SparseGcnSet2SetEncoder":
        from .sparse import SparseGcnSet2SetEncoder
        return SparseGcnSet2SetEncoder
    if name == "EdgeAttention":
        from .sparse import EdgeAttention
        return EdgeAttention
    if name == "GatConv":
        from .sparse import GatConv
        return GatConv
    if name in ("SageConv", "SageEncoder", "TopKPooling", "NestedSageEncoder"):
        from . import sparse
        return getattr(sparse, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
