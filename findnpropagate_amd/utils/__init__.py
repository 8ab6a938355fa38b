from . import loss_utils

__all__ = ["loss_utils"]
