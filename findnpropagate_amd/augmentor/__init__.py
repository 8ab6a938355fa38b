from . import data_augmentor, database_sampler, pseudo_loader

__all__ = ["data_augmentor", "database_sampler", "pseudo_loader"]
