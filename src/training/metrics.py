"""src.training.metrics (reference src/training/metrics.py) -> ncf_amd.metrics."""
from ncf_amd.metrics import full_rank_metrics, metrics  # noqa: F401
