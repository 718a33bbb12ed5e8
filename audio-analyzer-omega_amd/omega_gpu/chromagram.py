"""ChromagramAnalyzer.compute_chromagram over libomega.so (omega4/panels/chromagram.py:109-237).

The per-frame work (harmonic suppression, the 12 x K Gaussian pitch-class projection, smoothing,
normalisation) runs on the device; the genre-dependent temporal blend with the previous frame
(:215-237) is 12 multiply-adds and stays with the stateful caller object, as in the reference.
The tuning offset (:111-113, :128-129) is a whole number of semitones added to every bin's MIDI
number, so it rotates the 12 classes: the device computes the offset-0 chroma and the facade rolls it
(smoothing and normalisation commute with the rotation). The offset itself (detect_tuning_offset,
:581-639, metal / rock only) is a peak pick over the handful of 70-100 Hz bins of each frame plus a
30-deep mode -- scalar host logic, like the reference's.
Key, alternative-key, chord and mode scores (:239-339, :396-418, :670-812, music_theory.py:175-200) come from
omega_tonal_features / omega_tonal_spectra as one row per frame (include/omega.h has the columns); the histories, the
names and the rules that read them -- the flat-chroma fallback, the metal riff pattern, anti-stick's repeat count, the
history-append rule -- are host logic here, as in the reference. ChromagramPanel (:937-1214, without pygame and
draw) ties them together; update_batch runs the frames of one stream through one omega_tonal_spectra call.
"""
from __future__ import annotations

import ctypes as C
import logging
from collections import Counter, deque
from typing import Any, Dict, List, Optional, Tuple

import numpy as np

from . import _lib as L
from .engine import utility_engine
from .music_theory import MusicTheory

_BLEND = {"metal": 0.7, "rock": 0.7, "jazz": 0.5}
_E2 = 82.41  # chromagram.py:592-599: E2 and the drop tunings' lowest-string references
_TUNINGS = ((0, _E2), (-1, _E2 * 0.944), (-2, _E2 * 0.891), (-3, _E2 * 0.841), (-4, _E2 * 0.794))
logger = logging.getLogger(__name__)

# omega_tonal_features' row (include/omega.h)
COLS, STATE_LEN = 52, 13
FLAG_NONFINITE, FLAG_ZERO, FLAG_FLAT = 1, 2, 4
GENRES = ("pop", "jazz", "classical", "metal", "rock", "other")
MODE_NAMES = list(MusicTheory.MODES)


class ChromagramAnalyzer:
    def __init__(self, sample_rate: int = 48000, device: int = 0):
        self._host_init(sample_rate)
        self._eng = utility_engine(sample_rate, device)
        assert L.lib().omega_tonal_state_size() == STATE_LEN

    def _host_init(self, sample_rate: int = 48000) -> None:
        """Everything but the engine (:22-107): a new analyzer's histories, tuning state and genre."""
        self.sample_rate = sample_rate
        self.chroma_bins = 12
        self.transposition_offset = 0
        self.chroma_history = deque(maxlen=8)
        self.current_genre = "pop"
        self.tuning_history = []
        self.note_names = list(MusicTheory.NOTE_NAMES)
        self.chord_types = {
            'major': [0, 4, 7], 'minor': [0, 3, 7], 'dim': [0, 3, 6], 'aug': [0, 4, 8], 'maj7': [0, 4, 7, 11],
            'min7': [0, 3, 7, 10], 'dom7': [0, 4, 7, 10], 'maj9': [0, 4, 7, 11, 2], 'min9': [0, 3, 7, 10, 2],
            '13': [0, 4, 7, 10, 2, 5, 9], 'power': [0, 7], 'sus2': [0, 2, 7], 'sus4': [0, 5, 7]}
        self._type_names = list(self.chord_types)
        self.key_history = deque(maxlen=30)
        self.chord_history = deque(maxlen=50)
        self.mode_history = deque(maxlen=30)
        self.modulation_history = deque(maxlen=100)
        self.roman_numeral_sequence = deque(maxlen=16)
        self.chord_transition_matrix = {}
        self._configured = None
        self._cache = None  # (chroma bytes, genre id) -> the single-frame row and alternative correlations

    # -- the device part --
    def _genre_id(self) -> int:
        g = self.current_genre.lower()
        return GENRES.index(g) if g in GENRES[:5] else 5

    def _configure(self) -> None:
        g = self._genre_id()
        if self._configured != g:
            self._eng._check(L.lib().omega_tonal_configure(self._eng._ctx, C.byref(L.TonalConfig(g))))
            self._configured = g

    @staticmethod
    def _args(F, roll, first, state):
        roll = None if roll is None else np.ascontiguousarray(roll, np.int32)
        first = None if first is None else np.ascontiguousarray(first, np.int32)
        state = None if state is None else np.ascontiguousarray(state, np.float64)
        if any(a is not None and len(a) != F for a in (roll, first)) or (state is not None and state.size != STATE_LEN):
            raise ValueError(f"roll and first hold one value per frame, the state {STATE_LEN}")
        ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        return (roll, first, state), (ptr(roll), ptr(first), ptr(state))

    def tonal_rows(self, raw, roll=None, first=None, state=None, details: bool = False):
        """omega_tonal_features on host rows [F, 12] of raw chroma in the current genre -> (rows [F, 52], the new
        state, and with details the (key_corr, alt_corr, chord, mode) matrices). Nothing of this object changes."""
        raw = np.ascontiguousarray(np.atleast_2d(raw), np.float64)
        F = len(raw)
        if raw.shape[1] != 12:
            raise ValueError("raw chroma must be [F, 12]")
        keep, ptrs = self._args(F, roll, first, state)
        self._configure()
        rows, new = np.empty((F, COLS)), np.empty(STATE_LEN)
        det = [np.empty((F,) + s) for s in ((24,), (24,), (2, 12, 13), (12, 7))] if details else [None] * 4
        self._eng._check(L.lib().omega_tonal_features(
            self._eng._ctx, raw.ctypes.data, F, *ptrs, new.ctypes.data, rows.ctypes.data,
            *(None if d is None else d.ctypes.data for d in det), L.MEM_HOST))
        return (rows, new, tuple(det)) if details else (rows, new)

    def tonal_spectra(self, spectra, df, roll=None, first=None, state=None):
        """omega_tonal_spectra on host spectra [F, K]: chroma and scores in one call -> (rows [F, 52], new state)."""
        spectra = np.ascontiguousarray(np.atleast_2d(spectra), np.float32)
        F, K = spectra.shape
        keep, ptrs = self._args(F, roll, first, state)
        self._configure()
        rows, new = np.empty((F, COLS)), np.empty(STATE_LEN)
        self._eng._check(L.lib().omega_tonal_spectra(
            self._eng._ctx, spectra.ctypes.data, F, K, float(df), *ptrs, new.ctypes.data, rows.ctypes.data,
            None, None, None, None, L.MEM_HOST))
        return rows, new

    def _row(self, chroma):
        """The single-frame row of a caller's chroma (first set: nothing is blended), with its alternative
        correlations; detect_key, detect_chord and get_alternative_keys of one frame share one library call."""
        chroma = np.ascontiguousarray(chroma, np.float64)
        key = (chroma.tobytes(), self._genre_id())
        if self._cache is None or self._cache[0] != key:
            rows, _, det = self.tonal_rows(chroma[None, :], first=[1], details=True)
            self._cache = (key, rows[0], det[1][0])
        return self._cache[1], self._cache[2]

    # -- names --
    def _key_name(self, k: int) -> str:
        return f"{self.note_names[k // 2]} {'Minor' if k % 2 else 'Major'}"

    def _chord_name(self, cell: int) -> str:
        if cell < 0:
            return "N/A"
        name = self._type_names[cell % 13]
        return self.note_names[cell // 13] + ("5" if name == "power" else name)

    # -- the reference's surface on one frame --
    def detect_key(self, chroma: np.ndarray) -> Tuple[str, float]:
        """:239-339."""
        return self._key_from_row(self._row(chroma)[0])

    def _key_from_row(self, row) -> Tuple[str, float]:
        flags = int(row[12])
        if flags & FLAG_ZERO:
            return "Unknown", 0.0
        if flags & FLAG_FLAT:
            chord_key = self._detect_key_from_chords()
            return (chord_key, 0.5) if chord_key else ("Unknown", 0.0)
        key, corr = self._key_name(int(row[14])), row[15]
        self.key_history.append((key, corr))
        return key, corr

    def get_key_stability(self) -> float:
        """:341-356."""
        if len(self.key_history) < 10:
            return 0.0
        counts = Counter(k for k, _ in self.key_history)
        return max(counts.values()) / len(self.key_history)

    def get_most_likely_key(self) -> Tuple[str, float]:
        """:358-394."""
        if not self.key_history:
            return "Unknown", 0.0
        if len(self.chord_history) >= 4:
            chord_key = self._detect_key_from_chords()
            if chord_key and chord_key != "Unknown":
                self.key_history.append((chord_key, 0.85))
        weighted: Dict[str, Any] = {}
        n = len(self.key_history)
        for i, (key, corr) in enumerate(self.key_history):
            weighted[key] = weighted.get(key, 0) + corr * ((i + 1) / n)
        best = max(weighted, key=weighted.get)
        total = sum(weighted.values())
        confidence = weighted[best] / total if total > 0 else 0.0
        if confidence < 0.3:
            chord_key = self._detect_key_from_chords()
            if chord_key and chord_key != "Unknown":
                return chord_key, 0.6
            return "Unknown", confidence
        return best, confidence

    def get_alternative_keys(self, chroma: np.ndarray, top_n: int = 3) -> List[Tuple[str, float]]:
        """:396-418."""
        alt = self._row(chroma)[1]
        order = sorted(range(24), key=lambda k: -alt[k])  # (stable: equal scores keep the key order)
        return [(self._key_name(k), alt[k]) for k in order[:top_n]]

    def _alternatives_from_row(self, row):
        return [(self._key_name(int(row[16 + q])), row[19 + q]) for q in range(3)]

    def _detect_key_from_chords(self) -> Optional[str]:
        """:420-509."""
        if len(self.chord_history) < 4:
            return None
        recent = [c for c in list(self.chord_history)[-12:] if c != 'N/A']
        if len(recent) < 3:
            return None
        roots: Dict[str, int] = {}
        has_major = has_minor = False
        for chord in recent:
            if len(chord) >= 2:
                cut = 2 if chord[1] in '#b' else 1
                root, kind = chord[:cut], chord[cut:]
                roots[root] = roots.get(root, 0) + 1
                if 'maj' in kind.lower() or kind in ('', '5'):
                    has_major = True
                elif 'min' in kind.lower() or 'm' in kind:
                    has_minor = True
        if not roots:
            return None
        common = max(roots, key=roots.get)
        if 'F#' in roots and 'D' in roots:
            if roots['F#'] > roots['D'] * 1.5:
                return 'F# Minor' if has_minor else 'F# Major'
            return 'D Major'
        if 'C#' in roots and 'A' in roots:
            return 'A Major'
        fifth = self.note_names[(self.note_names.index(common) + 7) % 12] if common in self.note_names else None
        if fifth in roots:
            if has_major:
                return f"{common} Major"
            if has_minor:
                return f"{common} Minor"
        if roots[common] >= 3:
            return f"{common} Minor" if has_minor and not has_major else f"{common} Major"
        return None

    def _detect_metal_riff_pattern(self, chroma: np.ndarray, debug_enabled: bool = False) -> Optional[str]:
        """:511-579: the C#5 / D5 alternation of a drop-tuned riff, decided on four chroma values and the history."""
        cs, d, fs, gs, a = chroma[1], chroma[2], chroma[6], chroma[8], chroma[9]
        cs_power = cs > 0.1 and gs > 0.05
        d_power = d > 0.1 and a > 0.05
        recent = list(self.chord_history)[-10:]
        n_cs = sum(1 for c in recent if 'C#' in c or 'Db' in c)
        n_d = sum(1 for c in recent if c.startswith('D') and 'D#' not in c and 'Db' not in c)
        if cs_power and d_power:
            return "D5" if n_cs > n_d else "C#5"
        if cs_power and cs > d * 1.5:
            return "C#5"
        if d_power and d > cs * 1.5:
            return "D5"
        if fs > 0.2 and (cs_power or d_power) and (cs > 0.08 or d > 0.08):
            return "C#5" if n_cs <= n_d else "D5"
        return None

    def detect_chord(self, chroma: np.ndarray, debug_enabled: bool = False) -> Tuple[str, float]:
        """:656-839."""
        if self.current_genre.lower() == 'metal':  # (decided before anything is scored)
            riff = self._detect_metal_riff_pattern(chroma, debug_enabled)
            if riff:
                return riff, 0.9
        return self._chord_from_row(self._row(chroma)[0], chroma, debug_enabled, riff_done=True)

    def _chord_from_row(self, row, chroma, debug_enabled: bool = False, riff_done: bool = False) -> Tuple[str, float]:
        genre = self.current_genre.lower()
        if genre == 'metal' and not riff_done:
            riff = self._detect_metal_riff_pattern(chroma, debug_enabled)
            if riff:
                return riff, 0.9
        cell = int(row[22])
        best_chord, best_score = self._chord_name(cell), (row[23] if cell >= 0 else 0.0)
        if genre in ('metal', 'rock'):
            same = 0
            for c in reversed(self.chord_history):
                if c != best_chord:
                    break
                same += 1
            # anti-stick (:779-822): the second entry of the device's sorted second matrix, when close enough
            if same > 10 and int(row[26]) >= 0 and row[27] > row[25] * 0.85:
                best_chord, best_score = self._chord_name(int(row[26])), row[27]
        if not self.chord_history or best_chord != self.chord_history[-1] or best_score > 0.6:
            self.chord_history.append(best_chord)
        return best_chord, best_score

    def get_chord_progression(self) -> List[str]:
        return list(self.chord_history)[-8:]

    def analyze_harmonic_rhythm(self) -> float:
        """:845-853."""
        h = list(self.chord_history)
        if len(h) < 2:
            return 0.0
        return sum(1 for a, b in zip(h[:-1], h[1:]) if a != b) / (len(h) - 1)

    def get_enhanced_chord_progression(self) -> List[str]:
        """:855-892: short histories padded from a common progression in the current key."""
        chords = list(self.chord_history)
        key = getattr(self, 'current_key', None)
        if len(chords) < 8 and key and key != 'Unknown':
            root = key.split()[0]
            t = self._transpose_chord
            if 'Major' in key:
                prog = [root + 'major', root + 'major', t(root, 5, 'major'), t(root, 9, 'minor'), t(root, 5, 'major'),
                        t(root, 3, 'major'), root + 'major', root + 'major']
            else:
                prog = [root + 'minor', root + 'minor', t(root, 10, 'major'), t(root, 8, 'major'), t(root, 10, 'major'),
                        t(root, 5, 'minor'), root + 'minor', root + 'minor']
            while len(chords) < 8:
                chords.append(prog[len(chords) % len(prog)])
        return chords[-8:]

    def _transpose_chord(self, root: str, semitones: int, chord_type: str) -> str:
        if root not in self.note_names:
            return root + chord_type
        return self.note_names[(self.note_names.index(root) + semitones) % 12] + chord_type

    def set_genre_context(self, genre: str):
        self.current_genre = genre

    def transpose_chord_name(self, chord_name: str, semitones: int) -> str:
        """:907-934."""
        if chord_name == 'N/A':
            return chord_name
        cut = 2 if len(chord_name) > 1 and chord_name[1] in '#b' else 1
        root, kind = chord_name[:cut], chord_name[cut:]
        if root not in self.note_names:
            return chord_name
        return self.note_names[(self.note_names.index(root) + semitones) % 12] + kind

    def _raw(self, spectra: np.ndarray, freqs: np.ndarray) -> np.ndarray:
        spectra = np.atleast_2d(spectra)
        df = float(freqs[1] - freqs[0]) if len(freqs) > 1 else float(self.sample_rate) / 2
        return self._eng.chroma_raw(spectra, df)

    @staticmethod
    def _find_peaks(data: np.ndarray, prominence: float = 0.3) -> np.ndarray:
        """chromagram.py:641-654."""
        if len(data) < 3:
            return np.array([], int)
        thr = np.max(data) * prominence
        inner = data[1:-1]
        return np.nonzero((inner > data[:-2]) & (inner > data[2:]) & (inner > thr))[0] + 1

    def detect_tuning_offset(self, fft_data: np.ndarray, freqs: np.ndarray) -> int:
        """chromagram.py:581-639: the first 70-100 Hz peak against the tuning references (closest
        within 50 cents, else standard), then the mode of the last 30 detections once there are 5."""
        sel = (freqs > 70) & (freqs < 100)
        bass = np.asarray(fft_data)[sel]
        if len(bass) == 0:
            return self.transposition_offset
        pk = self._find_peaks(bass, 0.3)
        if len(pk) == 0:
            return self.transposition_offset
        pf = freqs[sel][pk[0]]
        best, dmin = 0, float("inf")
        for off, rf in _TUNINGS:
            if pf > 0 and rf > 0:
                d = abs(1200 * np.log2(pf / rf))
                if d < dmin and d < 50:
                    best, dmin = off, d
        self.tuning_history.append(best)
        if len(self.tuning_history) > 30:
            self.tuning_history.pop(0)
        if len(self.tuning_history) >= 5:
            return Counter(self.tuning_history).most_common(1)[0][0]
        return best

    def _offsets(self, spectra: np.ndarray, freqs: np.ndarray) -> np.ndarray:
        """The transposition offset in force for each frame, in order (state advanced)."""
        offs = np.empty(len(spectra), int)
        detect = self.current_genre.lower() in ("metal", "rock")
        for f in range(len(spectra)):
            if detect:
                self.transposition_offset = self.detect_tuning_offset(spectra[f], freqs)
            offs[f] = self.transposition_offset
        return offs

    def _chroma(self, spectra: np.ndarray, freqs: np.ndarray) -> np.ndarray:
        spectra = np.atleast_2d(np.asarray(spectra, np.float32))
        offs = self._offsets(spectra, freqs)
        raw = self._raw(spectra, freqs)
        for f in np.nonzero(offs)[0]:
            raw[f] = np.roll(raw[f], int(offs[f]))
        return raw

    def _blend(self):
        if len(self.chroma_history) == 0:
            return np.zeros(12)
        cur = self.chroma_history[-1]
        if len(self.chroma_history) == 1:
            return cur
        a = _BLEND.get(self.current_genre.lower(), 0.3)
        return self.chroma_history[-2] * (1 - a) + cur * a

    def compute_chromagram(self, fft_data: np.ndarray, freqs: np.ndarray) -> np.ndarray:
        """chromagram.py:109-159. Errors are logged and the last blended chroma returned."""
        try:
            raw = self._chroma(fft_data, np.asarray(freqs))[0]
        except Exception as e:
            logger.error("compute_chromagram failed: %s", e)
            return self._blend()
        self.chroma_history.append(raw.copy())
        return self._blend()

    def compute_chromagram_batch(self, spectra: np.ndarray, freqs: np.ndarray) -> np.ndarray:
        """Frames of one stream in order: [F, K] -> [F, 12] blended chroma, state advanced."""
        raw = self._chroma(spectra, np.asarray(freqs))
        out = np.empty_like(raw)
        for f in range(len(raw)):
            self.chroma_history.append(raw[f].copy())
            out[f] = self._blend()
        return out


def _blank_info() -> Dict[str, Any]:
    return {'chromagram': np.zeros(12), 'key': 'Unknown', 'is_major': True, 'confidence': 0.0, 'stability': 0.0,
            'alternative_keys': [], 'current_chord': 'N/A', 'chord_confidence': 0.0, 'chord_progression': [],
            'harmonic_rhythm': 0.0, 'mode': 'Ionian (Major)', 'mode_confidence': 0.0, 'roman_progression': [],
            'key_modulation': None, 'chord_transitions': {}}


class ChromagramPanel:
    """ChromagramPanel (:937-1214) without pygame: update() / update_batch() and get_results(). Every frame's
    chroma, blend and scores come from one omega_tonal_spectra call per batch; the loop over its rows is host logic."""

    def __init__(self, sample_rate: int = 48000, device: int = 0):
        self.analyzer = ChromagramAnalyzer(sample_rate, device)
        self._host_init(sample_rate)

    def _host_init(self, sample_rate: int = 48000) -> None:
        self.sample_rate = sample_rate
        self.chromagram_info = _blank_info()
        self.chromagram = np.zeros(12)
        self.detected_key = 'Unknown'
        self.key_confidence = 0.0
        self.current_chord = 'N/A'
        self.chord_confidence = 0.0
        self.chord_sequence = []
        self.circle_position = 0
        self.current_mode = 'Ionian (Major)'
        self.mode_confidence = 0.0
        self.key_modulation = None
        self.roman_progression = []
        self.chord_transition_matrix = {}

    def set_fonts(self, fonts) -> None:
        """Accepted and ignored: nothing is drawn."""

    def reset(self) -> None:
        """A new panel on the same context: every history, the tuning state and the displayed values."""
        self.analyzer._host_init(self.analyzer.sample_rate)
        self._host_init(self.sample_rate)

    def _silence(self) -> None:
        """:1000-1044."""
        an = self.analyzer
        kept = self.chord_transition_matrix  # (the reference clears the displayed copy only)
        self._host_init(self.sample_rate)
        self.chord_transition_matrix = kept
        self.key_stability = 0.0
        self.alternative_keys = []
        self.chord_progression = []
        self.harmonic_rhythm = 0.0
        for h in (an.chroma_history, an.chord_history, an.key_history, an.mode_history, an.modulation_history,
                  an.roman_numeral_sequence):
            h.clear()

    def update(self, fft_data, audio_data, freqs, current_genre: str = None, debug_enabled: bool = False) -> None:
        """:990-1206."""
        if fft_data is None or len(fft_data) == 0:
            return
        self._run(np.asarray(fft_data)[None, :], None if audio_data is None else [np.asarray(audio_data)], freqs,
                  current_genre, debug_enabled)

    def update_batch(self, spectra, audio, freqs, current_genre: str = None) -> List[Dict[str, Any]]:
        """The frames [F, K] of one stream in order (audio: F frames or None), as F update() calls with one genre:
        one library call for the frames that are not silent, then get_results() after each frame."""
        spectra = np.asarray(spectra)
        if spectra.ndim != 2:
            raise ValueError("spectra must be [F, K]")
        if spectra.shape[1] == 0:
            return [self.get_results() for _ in range(len(spectra))]
        return self._run(spectra, audio, freqs, current_genre, False)

    def _run(self, spectra, audio, freqs, current_genre, debug_enabled) -> List[Dict[str, Any]]:
        an = self.analyzer
        F = len(spectra)
        silent = np.zeros(F, bool)
        if audio is not None:
            for f in range(F):
                silent[f] = np.sqrt(np.mean(audio[f] ** 2)) < 0.001  # (:999-1000, in the frame's own dtype)
        live = np.nonzero(~silent)[0]
        rows = offs = None
        if len(live):
            an.set_genre_context(current_genre if current_genre and current_genre != 'Unknown' else 'pop')
            freqs = np.asarray(freqs)
            spec = np.ascontiguousarray(spectra[live], np.float32)
            offs = an._offsets(spec, freqs)
            # a frame behind a silent one, or a stream's first, has no predecessor
            first = np.zeros(len(live), np.int32)
            first[1:] = silent[live[1:] - 1]
            carry = None
            if silent[:live[0]].any() or len(an.chroma_history) == 0:
                first[0] = 1
            else:
                carry = np.concatenate(([1.0], an.chroma_history[-1]))
            df = float(freqs[1] - freqs[0]) if len(freqs) > 1 else float(an.sample_rate) / 2
            rows, state = an.tonal_spectra(spec, df, offs, first, carry)
        out, j = [], 0
        for f in range(F):
            if silent[f]:
                self._silence()
            else:
                self._step(rows[j], int(offs[j]), debug_enabled)
                j += 1
            out.append(self.get_results())
        if len(live) and not silent[live[-1] + 1:].any():
            an.chroma_history.append(state[1:].copy())  # the newest raw row: all the next blend reads
        return out

    def _step(self, row, offset: int, debug_enabled: bool) -> None:
        """:1077-1206 on one frame's row."""
        an = self.analyzer
        chromagram = row[:12].copy()
        key, correlation = an._key_from_row(row)
        chord, chord_conf = an._chord_from_row(row, chromagram, debug_enabled)
        display_chord = chord
        if offset != 0 and chord != 'N/A':
            display_chord = an.transpose_chord_name(chord, -offset)
        stability = an.get_key_stability()
        most_likely_key, confidence = an.get_most_likely_key()
        alt_keys = an._alternatives_from_row(row)
        an.current_key = most_likely_key
        chord_progression = an.get_chord_progression()
        harmonic_rhythm = an.analyze_harmonic_rhythm()
        self.circle_position, _ = MusicTheory.get_circle_position(most_likely_key)
        root = self._get_root_index(most_likely_key)
        mode, mode_conf = MODE_NAMES[int(row[28 + root])], row[40 + root]
        an.mode_history.append((mode, mode_conf))
        if len(an.mode_history) > 5:
            mode_conf = np.mean([c for _, c in an.mode_history])
            mode = max(set(m for m, _ in an.mode_history), key=lambda x: sum(1 for m, _ in an.mode_history if m == x))
        roman_progression = []
        for name in chord_progression[-8:]:
            roman = MusicTheory.chord_to_roman(name, most_likely_key)
            roman_progression.append(roman)
            an.roman_numeral_sequence.append(roman)
        self.key_modulation = None
        if len(an.modulation_history) > 0 and an.modulation_history[-1] != most_likely_key:
            self.key_modulation = MusicTheory.detect_key_modulation(an.modulation_history[-1], most_likely_key)
        an.modulation_history.append(most_likely_key)
        if len(chord_progression) > 1:
            self.chord_transition_matrix = MusicTheory.create_chord_transition_matrix(list(an.roman_numeral_sequence))
        self.chromagram_info = {
            'chromagram': chromagram, 'key': most_likely_key, 'is_major': 'Major' in most_likely_key,
            'confidence': confidence, 'stability': stability,
            'alternative_keys': [(k, c) for k, c in alt_keys[1:] if c > 0.3], 'current_chord': display_chord,
            'chord_confidence': chord_conf, 'chord_progression': chord_progression, 'harmonic_rhythm': harmonic_rhythm,
            'mode': mode, 'mode_confidence': mode_conf, 'roman_progression': roman_progression,
            'key_modulation': self.key_modulation, 'chord_transitions': self.chord_transition_matrix}
        self.chromagram = chromagram.copy()
        self.detected_key = most_likely_key
        self.key_confidence = confidence
        self.current_chord = display_chord
        self.chord_confidence = chord_conf
        self.chord_sequence = chord_progression
        self.current_mode = mode
        self.mode_confidence = mode_conf
        self.roman_progression = roman_progression

    def _get_root_index(self, key: str) -> int:
        root = key.split()[0]
        return MusicTheory.NOTE_NAMES.index(root) if root in MusicTheory.NOTE_NAMES else 0

    def get_results(self) -> Dict[str, Any]:
        return self.chromagram_info.copy()
