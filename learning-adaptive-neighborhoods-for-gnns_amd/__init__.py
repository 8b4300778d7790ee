"""MI355X-native Differentiable Graph Generator hot path (package directory:
`learning-adaptive-neighborhoods-for-gnns_amd/`, importable as `dgg_amd` through the shim at the repo root).

Public surface mirrors the reference's modules:
    dgg_amd.dgm.{DGG_LearnableK_debug, DGG, LearnableKEncoder}               (reference dgm.py)
    dgg_amd.model.{GCNConv, GraphConvolution, DenseGraphConvolution, GCN_DGG, GCN_DGG_00, GCNII_DGG, GCNIIppi_DGG}  (model.py)
    dgg_amd.distributed.{ShardedGCN_DGG, global_nll_loss}                    (GCN_DGG row-sharded across GPUs)
plus the containers `AllPairs` / `EllAdjacency` / `CsrAdjacency`, the raw kernel wrappers in `dgg_amd.ops` and `ScalarLog`, a
dependency-free writer for the models' `writer=` argument, and `adjacency_mse_loss`, the reference's supervision of the learned adjacency
(train_reddit.py:236-251) on sparse rows (target: `dgg_amd.data.remove_interclass_edges`).  Mini-batches of one large graph come
from `RandomWalkSampler` / `ClusterSampler` (dgg_amd.sampling: the reference's GraphSAINTRandomWalkSampler / ClusterLoader,
train_large_graphs.py:402-421), each batch a `SubgraphBatch`; `SubgraphBatch.with_noise` gives the `EditedBatch` with the reference's per-batch noisy edges and the
same-class target of the adjacency loss, built on the device (ops.batch_graph_edit); `dgg_amd.train_large_graphs` is the harness on
top of them.
"""
from . import _lib, ops  # noqa: F401
from .adjacency import (AllPairs, CsrAdjacency, EllAdjacency, adjacency_mse_loss, csr_candidates, csr_pattern,  # noqa: F401
                        ell_from_dense)
from .dgm import (DGG, DGG_Ablations, DGG_LearnableK_debug, DGG_LearnableK_SDD, DGG_StraightThrough,  # noqa: F401
                  LearnableKEncoder)
from .model import (DenseGraphConv, DenseGraphConvolution, GAT_DGG_00, GAT_DGG_Ablations, GATConv_DGG, GCN_DGG, GCN_DGG_00,  # noqa: F401
                    GCN_DGG_Ablations, GCNConv, GCNII_DGG, GCNIIppi_DGG,
                    GraphConvolution, SAGE_DGG, SAGE_DGG_00)
from .distributed import ShardedGCN_DGG, global_nll_loss  # noqa: F401
from .scalar_log import ScalarLog  # noqa: F401
from .sampling import ClusterSampler, EditedBatch, RandomWalkSampler, SubgraphBatch, contiguous_parts  # noqa: F401
