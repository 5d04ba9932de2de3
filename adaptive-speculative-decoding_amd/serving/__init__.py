"""Serving-side mirror of the reference's src/serving package (the pipeline and the stages behind it; the HTTP
shell and the cost optimiser are out of scope)."""
from .cache import RequestCache  # noqa: F401
from .components import FeatureExtractor, QualityPredictor  # noqa: F401
from .pipeline import AdaptiveSpeculativePipeline, PipelineConfig, RequestResult  # noqa: F401
from .stages import Stage, StageConfig, StageManager  # noqa: F401
