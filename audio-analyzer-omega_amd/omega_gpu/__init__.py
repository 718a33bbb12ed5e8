"""omega_gpu -- MI355X engine for the OMEGA-4 analysis hot path, behind the reference's own Python
surfaces (see include/omega.h for the C ABI and the reference file:line each entry point replaces).

Everything numeric runs in libomega.so (hand-written HIP for gfx950); importing a facade without the
built library raises ImportError -- there is no CPU fallback.
"""
from ._lib import LIB_PATH, OmegaError, UnsupportedError, lib
from .engine import DEFAULT_RESOLUTIONS, METER_KEYS, NORTHSTAR_RESOLUTIONS, BandTable, Engine, Resolution
from .pitch_detection import CepstralAnalyzer, PitchDetectionConfig, get_preset_config, list_presets
from .harmonic_analysis import HarmonicAnalyzer, HarmonicMetrics
from .genre_classification import GenreClassifier
from .hip_hop_detector import HipHopDetector
from .phase_correlation import PhaseCorrelation
from .room_modes import RoomModeAnalyzer, RoomModeConfig
from .voice_detection import VoiceDetectionPanel
from .transient_detection import TransientDetectionPanel
from .bass_zoom import BassZoomPanel
from .beat_detection import BeatDetectionPanel, BeatDetector
from .frequency_band_tracker import FrequencyBandTracker, FrequencyBandTrackerPanel
from .spectrogram_waterfall import SpectrogramWaterfall, SpectrogramWaterfallPanel
from .chromagram import ChromagramAnalyzer, ChromagramPanel
from .music_theory import MusicTheory
from .professional_meters import ProfessionalMetersPanel

__all__ = [
    "SpectrogramWaterfall", "SpectrogramWaterfallPanel", "ChromagramAnalyzer", "ChromagramPanel", "MusicTheory",
    "HarmonicAnalyzer", "HarmonicMetrics", "GenreClassifier", "HipHopDetector", "PhaseCorrelation",
    "RoomModeAnalyzer", "RoomModeConfig", "VoiceDetectionPanel", "TransientDetectionPanel", "BassZoomPanel",
    "ProfessionalMetersPanel", "BeatDetector", "BeatDetectionPanel", "FrequencyBandTracker", "FrequencyBandTrackerPanel",
    "LIB_PATH", "OmegaError", "UnsupportedError", "lib", "Engine", "Resolution", "BandTable",
    "DEFAULT_RESOLUTIONS", "NORTHSTAR_RESOLUTIONS", "METER_KEYS",
    "CepstralAnalyzer", "PitchDetectionConfig", "get_preset_config", "list_presets",
]
