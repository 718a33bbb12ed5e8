"""MusicTheory (omega4/panels/music_theory.py): the constants and static helpers the chromagram panel reads --
circle of fifths, relative keys, Roman numerals, modes, modulation types, chord transitions. Pure host code on
strings and 12 numbers; ChromagramPanel takes analyze_mode's scores for a batch of frames from the device
(omega_tonal_features computes every root), a single call here stays numpy.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np


class MusicTheory:
    CIRCLE_OF_FIFTHS = ['C', 'G', 'D', 'A', 'E', 'B', 'F#', 'C#', 'G#', 'D#', 'A#', 'F']
    CIRCLE_OF_FIFTHS_MINOR = ['Am', 'Em', 'Bm', 'F#m', 'C#m', 'G#m', 'D#m', 'A#m', 'Fm', 'Cm', 'Gm', 'Dm']
    NOTE_NAMES = ['C', 'C#', 'D', 'D#', 'E', 'F', 'F#', 'G', 'G#', 'A', 'A#', 'B']
    FLAT_NAMES = ['C', 'Db', 'D', 'Eb', 'E', 'F', 'Gb', 'G', 'Ab', 'A', 'Bb', 'B']
    MODES = {  # intervals from the root, in the order analyze_mode tests them
        'Ionian (Major)': [0, 2, 4, 5, 7, 9, 11],
        'Dorian': [0, 2, 3, 5, 7, 9, 10],
        'Phrygian': [0, 1, 3, 5, 7, 8, 10],
        'Lydian': [0, 2, 4, 6, 7, 9, 11],
        'Mixolydian': [0, 2, 4, 5, 7, 9, 10],
        'Aeolian (Natural Minor)': [0, 2, 3, 5, 7, 8, 10],
        'Locrian': [0, 1, 3, 5, 6, 8, 10],
    }
    ROMAN_NUMERALS_MAJOR = ['I', 'ii', 'iii', 'IV', 'V', 'vi', 'vii°']
    ROMAN_NUMERALS_MINOR = ['i', 'ii°', 'III', 'iv', 'v', 'VI', 'VII']
    PROGRESSIONS = {
        'I-V-vi-IV': ['I', 'V', 'vi', 'IV'],
        'I-vi-IV-V': ['I', 'vi', 'IV', 'V'],
        'ii-V-I': ['ii', 'V', 'I'],
        'I-IV-V': ['I', 'IV', 'V'],
        'vi-IV-I-V': ['vi', 'IV', 'I', 'V'],
        'I-V-vi-iii-IV-I-IV-V': ['I', 'V', 'vi', 'iii', 'IV', 'I', 'IV', 'V'],
        'i-VII-VI-V': ['i', 'VII', 'VI', 'V'],
        'i-iv-V': ['i', 'iv', 'V'],
    }
    CHORD_FUNCTIONS = {
        'I': 'Tonic', 'ii': 'Supertonic', 'iii': 'Mediant', 'IV': 'Subdominant', 'V': 'Dominant', 'vi': 'Submediant',
        'vii°': 'Leading Tone', 'i': 'Tonic', 'ii°': 'Supertonic', 'III': 'Mediant', 'iv': 'Subdominant',
        'v': 'Dominant', 'VI': 'Submediant', 'VII': 'Subtonic',
    }
    TSD_GROUPS = {
        'Tonic': ['I', 'vi', 'iii', 'i', 'VI', 'III'],
        'Subdominant': ['IV', 'ii', 'iv', 'ii°'],
        'Dominant': ['V', 'vii°', 'v', 'VII'],
    }
    _ENHARMONIC = {'Gb': 'F#', 'Db': 'C#', 'Ab': 'G#', 'Eb': 'D#', 'Bb': 'A#'}

    @staticmethod
    def _shift(root: str, semitones: int, fallback: str) -> str:
        names = MusicTheory.NOTE_NAMES
        return names[(names.index(root) + semitones) % 12] if root in names else fallback

    @staticmethod
    def get_circle_position(key: str) -> Tuple[int, bool]:
        """:74-105: (position 0..11, is major); (0, True) for a root that is not on the circle."""
        if ' Major' in key:
            root, major = key.replace(' Major', ''), True
        elif ' Minor' in key:
            root, major = key.replace(' Minor', ''), False
        elif 'm' in key and len(key) <= 3:
            root, major = key.replace('m', ''), False
        else:
            root, major = key, True
        root = MusicTheory._ENHARMONIC.get(root, root)
        circle = MusicTheory.CIRCLE_OF_FIFTHS
        on = root if major else MusicTheory.relative_major(root)
        return (circle.index(on), major) if on in circle else (0, True)

    @staticmethod
    def relative_major(minor_root: str) -> str:
        return MusicTheory._shift(minor_root, 3, 'C')

    @staticmethod
    def relative_minor(major_root: str) -> str:
        return MusicTheory._shift(major_root, -3, 'A')

    @staticmethod
    def _split(chord: str) -> Tuple[str, str]:
        cut = 2 if len(chord) >= 2 and chord[1] in ('#', 'b') else 1
        return chord[:cut], chord[cut:]

    @staticmethod
    def chord_to_roman(chord: str, key: str) -> str:
        """:127-172: the scale degree's numeral with a 7 or 9 extension, an accidental with the chord's root for a
        root outside the scale, the chord itself where a root is unknown."""
        chord_root, quality = MusicTheory._split(chord)
        parts = key.split()
        major = len(parts) > 1 and parts[1] == 'Major'
        names = MusicTheory.NOTE_NAMES
        if parts[0] not in names or chord_root not in names:
            return chord
        degree = (names.index(chord_root) - names.index(parts[0])) % 12
        scale = [0, 2, 4, 5, 7, 9, 11] if major else [0, 2, 3, 5, 7, 8, 10]
        if degree in scale:
            numerals = MusicTheory.ROMAN_NUMERALS_MAJOR if major else MusicTheory.ROMAN_NUMERALS_MINOR
            roman = numerals[scale.index(degree)]
            return roman + ('7' if '7' in quality else ('9' if '9' in quality else ''))
        return f"♭{chord_root}" if degree - 1 in scale else f"♯{chord_root}"

    @staticmethod
    def analyze_mode(chroma: np.ndarray, root_idx: int) -> Tuple[str, float]:
        """:174-200: the first mode whose /7-normalised template correlates best, and above 0, with the chroma
        rotated to the root; ('Ionian (Major)', 0.0) otherwise."""
        best, score = 'Ionian (Major)', 0.0
        rotated = np.roll(chroma, -root_idx)
        if not np.std(rotated) > 0:
            return best, score
        for name, intervals in MusicTheory.MODES.items():
            template = np.zeros(12)
            template[intervals] = 1.0
            template = template / np.sum(template)
            c = np.corrcoef(rotated, template)[0, 1]
            if c > score:
                best, score = name, c
        return best, score

    @staticmethod
    def _base(roman: str) -> str:
        return roman.rstrip('7965')

    @staticmethod
    def get_chord_function(roman: str) -> str:
        return MusicTheory.CHORD_FUNCTIONS.get(MusicTheory._base(roman), 'Unknown')

    @staticmethod
    def get_tsd_group(roman: str) -> str:
        base = MusicTheory._base(roman)
        for group, members in MusicTheory.TSD_GROUPS.items():
            if base in members:
                return group
        return 'Other'

    @staticmethod
    def detect_key_modulation(prev_key: str, current_key: str) -> Optional[str]:
        """:220-266."""
        if prev_key == current_key:
            return None
        prev_root, cur_root = prev_key.split()[0], current_key.split()[0]
        prev_major, cur_major = 'Major' in prev_key, 'Major' in current_key
        if prev_root == cur_root:
            return "Parallel"
        if prev_major and not cur_major and MusicTheory.relative_minor(prev_root) == cur_root:
            return "Relative Minor"
        if cur_major and not prev_major and MusicTheory.relative_major(prev_root) == cur_root:
            return "Relative Major"
        circle = MusicTheory.CIRCLE_OF_FIFTHS
        if prev_root in circle and cur_root in circle:
            a, b = circle.index(prev_root), circle.index(cur_root)
            dist = min(abs(b - a), 12 - abs(b - a))
            if dist == 1:
                return "Dominant" if b == (a + 1) % 12 else "Subdominant"
            named = {2: "Supertonic", 3: "Mediant", 6: "Tritone"}
            if dist in named:
                return named[dist]
        return "Chromatic"

    @staticmethod
    def create_chord_transition_matrix(chord_sequence: List[str]) -> Dict[str, Dict[str, float]]:
        """:268-293: transition counts between neighbours, each row divided by its total."""
        counts: Dict[str, Dict[str, float]] = {}
        for cur, nxt in zip(chord_sequence[:-1], chord_sequence[1:]):
            row = counts.setdefault(cur, {})
            row[nxt] = row.get(nxt, 0) + 1
        for row in counts.values():
            total = sum(row.values())
            if total > 0:
                for nxt in row:
                    row[nxt] /= total
        return counts
