"""Drop-in surface of `reazonspeech.k2.asr` (pkg/k2-asr/src/__init__.py:1-4): TranscribeConfig, load_model, transcribe,
audio_from_numpy, audio_from_tensor, audio_from_path.  Additive: `transcribe_batch`, `align_text`, `align_text_batch`."""
from .interface import TranscribeConfig
from .huggingface import load_model
from .transcribe import transcribe, transcribe_batch
from .align import align_text, align_text_batch      # additive, like transcribe_batch; reached by name, not listed in __all__
from .align import score_texts, score_texts_batch    # additive: several candidate transcripts per audio on one lattice
from .audio import audio_from_numpy, audio_from_tensor, audio_from_path

__all__ = ["TranscribeConfig", "load_model", "transcribe", "transcribe_batch", "audio_from_numpy", "audio_from_tensor", "audio_from_path"]
