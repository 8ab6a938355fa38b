from . import centernet_utils, model_nms_utils, transfusion_utils

__all__ = ["centernet_utils", "model_nms_utils", "transfusion_utils"]
