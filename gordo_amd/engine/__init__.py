from .spec import ModelSpec, LayerSpec
from .pack import DensePack, LSTMPack, GRUPack, BasePack, pack_class

__all__ = ["ModelSpec", "LayerSpec", "DensePack", "LSTMPack", "GRUPack", "BasePack",
           "pack_class"]
