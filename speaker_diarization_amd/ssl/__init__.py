"""Self-supervised speech front ends on the HIP path."""
from .wavlm import WavLM, WavLMConfig, num_frames  # noqa: F401
