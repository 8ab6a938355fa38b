from . import data_augmentor, pseudo_loader

__all__ = ["data_augmentor", "pseudo_loader"]
