"""Drop-in mirror of the reference's ``rvc.infer`` package (infer.py + pipeline.py)."""
from .infer import Config, load_hubert, get_vc, rvc_infer, rvc_infer_many  # noqa: F401
from .pipeline import VC, PipelineHandle  # noqa: F401
