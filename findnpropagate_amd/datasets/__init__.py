"""Dataset-side pieces of the device input path (the reference's pcdet.datasets): what turns the files of a sample into the
arrays the device chain takes."""
from . import nuscenes_sweeps  # noqa: F401

__all__ = ["nuscenes_sweeps"]
