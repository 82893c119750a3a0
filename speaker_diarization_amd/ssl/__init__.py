"""Self-supervised speech front ends on the HIP path."""
from .wavlm import WavLM, WavLMConfig, num_frames  # noqa: F401
from .w2vbert import W2vBert, W2vBertConfig  # noqa: F401
from .whisper import WhisperEncoder, WhisperConfig  # noqa: F401
