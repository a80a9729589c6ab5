"""CPU: the host side of long recordings through `transcribe_batch` (espnet family): the lockstep planner cuts the windows the
REFERENCE's own loop cut (tests/golden/reference_espnet.json, produced by the reference's transcribe.py / ctc.py on the fake
model of tests/espnet_fake.py), with one `find_cuts` call per round, and the C ABI declares and exports the device blank
finder without a version bump."""
import ctypes
import importlib
import json
import os
import re

import numpy as np

import espnet_fake as fk

from reazonspeech_amd import build as rs_build
from reazonspeech_amd.espnet.asr import ctc
from reazonspeech_amd.runtime import capi

tr = importlib.import_module("reazonspeech_amd.espnet.asr.transcribe")

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = json.load(open(os.path.join(HERE, "golden", "reference_espnet.json")))
CASES = {"short_3s": (3.0, 1), "one_window_19s": (19.0, 2), "long_47s": (47.3, 3), "long_90s": (90.0, 4)}
WINDOW = 20 * 16000


def test_planner_in_lockstep_cuts_the_references_windows():
    names = list(CASES)
    wavs = [fk.long_audio(*CASES[name]) for name in names]
    wavs.append(np.zeros(0, np.float32))                     # a recording of length 0 rides along
    model = fk.FakeEspnetModel()
    rounds = []

    def find_cuts(requests):
        rounds.append(list(requests))
        assert all(n == WINDOW and o + n < len(wavs[i]) for i, o, n in requests)      # only recordings with MORE than a window left
        return [ctc.find_blank(model, wavs[i][o:o + n]) for i, o, n in requests]

    plan = tr.plan_windows([len(w) for w in wavs], WINDOW, find_cuts)
    assert len(plan) == len(wavs)
    for name, wav, pieces in zip(names, wavs, plan):
        assert [n for _, n in pieces] == GOLD["cases"][name]["windows"], name
        assert pieces[0][0] == 0 and all(o + n == o2 for (o, n), (o2, _) in zip(pieces, pieces[1:]))      # the pieces tile the recording
        assert pieces[-1][0] + pieces[-1][1] == len(wav)
    assert [len(GOLD["cases"][name]["windows"]) for name in names] == [1, 1, 3, 7]
    assert plan[-1] == []
    assert len(rounds) == 6                                  # seven pieces of the 90 s recording = six cuts = six rounds, not 2 + 6 calls
    assert [sorted(i for i, _, _ in r) for r in rounds] == [[2, 3], [2, 3], [3], [3], [3], [3]]
    for r in rounds:
        assert len({i for i, _, _ in r}) == len(r)           # a round never holds two windows of one recording


def test_planner_without_long_recordings_never_asks_for_cuts():
    def find_cuts(requests):
        raise AssertionError("no recording has more than a window left")
    assert tr.plan_windows([0, 1, WINDOW, 5], WINDOW, find_cuts) == [[], [(0, 1)], [(0, WINDOW)], [(0, 5)]]
    assert tr.plan_windows([], WINDOW, find_cuts) == []


def test_planner_takes_the_no_cut_fallback_as_a_whole_window():
    """find_blank's (n, n): the head is the whole window, and a rest of exactly one window is the last piece"""
    calls = []

    def find_cuts(requests):
        calls.append(len(requests))
        return [ctc.Blank(n, n) for _, _, n in requests]
    assert tr.plan_windows([250, 200, 101], 100, find_cuts) == [[(0, 100), (100, 100), (200, 50)], [(0, 100), (100, 100)], [(0, 100), (100, 1)]]
    assert calls == [3, 1]


def test_header_declares_and_library_exports_the_blank_finder():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rs_asr.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+rs_ctc_find_blank\s*\(\s*rs_ctx\s*\*\s*ctx\s*,\s*const\s+float\s*\*\s*blank_prob\s*,\s*const\s+int32_t\s*\*\s*enc_lens\s*,"
                     r"\s*const\s+int32_t\s*\*\s*n_samples\s*,\s*int\s+B\s*,\s*int\s+tp_max\s*,\s*float\s+threshold\s*,\s*int32_t\s*\*\s*cuts\s*,"
                     r"\s*void\s*\*\s*stream\s*\)", src)
    assert re.search(r"#define\s+RS_ABI_VERSION\s+7\b", src)
    lib = ctypes.CDLL(rs_build.build())
    assert hasattr(lib, "rs_ctc_find_blank")
    assert lib.rs_abi_version() == 7
    assert "rs_ctc_find_blank" in capi.EXPORTS
    lib.rs_ctc_find_blank.argtypes = capi.load().rs_ctc_find_blank.argtypes
    assert lib.rs_ctc_find_blank(None, None, None, None, 1, 4, 0.98, None, None) == capi.RS_EINVAL       # no context: refused, no crash
