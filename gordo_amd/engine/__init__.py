from .spec import ModelSpec, LayerSpec
from .pack import (DensePack, LSTMPack, GRUPack, Conv1DPack, BasePack,
                   pack_class)

__all__ = ["ModelSpec", "LayerSpec", "DensePack", "LSTMPack", "GRUPack", "Conv1DPack", "BasePack",
           "pack_class"]
