from .dist_agg import DistAgg, dist_aggregate, fp_exchange, qt_exchange
from .kernels import spmm, SpmmView, mixed_quantize, mixed_dequantize, native, has_native
from .norm_act import norm_relu_dropout, norm_relu_dropout_torch
from .loss import masked_loss, masked_loss_torch

__all__ = ['DistAgg', 'dist_aggregate', 'fp_exchange', 'qt_exchange',
           'spmm', 'SpmmView', 'mixed_quantize', 'mixed_dequantize',
           'native', 'has_native', 'norm_relu_dropout',
           'norm_relu_dropout_torch', 'masked_loss', 'masked_loss_torch']
