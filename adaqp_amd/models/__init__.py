from .gcn import DistGCN, DistGCNConv
from .sage import DistSAGE, DistSAGEConv
from .norm import FusedNormReluDropout

__all__ = ['DistGCN', 'DistGCNConv', 'DistSAGE', 'DistSAGEConv',
           'FusedNormReluDropout']
