"""`bindsnet.conversion`: a trained torch.nn model as a spiking network (reference: bindsnet/conversion)."""
from .conversion import FeatureExtractor, Permute, ann_to_snn, data_based_normalization, fold_batchnorm  # noqa: F401 (fold_batchnorm: an attribute, not in __all__)
from .nodes import PassThroughNodes, SubtractiveResetIFNodes
from .topology import ConstantPad2dConnection, PermuteConnection

__all__ = ["Permute", "FeatureExtractor", "data_based_normalization", "ann_to_snn", "SubtractiveResetIFNodes", "PassThroughNodes",
           "PermuteConnection", "ConstantPad2dConnection"]
