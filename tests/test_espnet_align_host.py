"""CPU: the host side of `segmentation="device"` (espnet family): the batch packer of the ground truths equals `prepare_text`
row for row, the C ABI declares and exports the aligner without a version bump, and a wrong mode is refused."""
import ctypes
import importlib
import itertools
import os
import re

import numpy as np
import pytest

from reazonspeech_amd import build as rs_build
from reazonspeech_amd.espnet.asr import ctc_segmentation as cs
from reazonspeech_amd.espnet.asr.model import synthetic_token_list
from reazonspeech_amd.runtime import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ABC = ["<blank>", "a", "b", "ab", "c", "abc"]


def check_pack(char_list, texts):
    """-> the packed batch, after checking every row against prepare_text on that text alone"""
    params = cs.CtcSegmentationParameters(char_list=list(char_list))
    gt, gt_lens, bounds = cs.pack_ground_truth(params, texts)
    S = max(len(c) for c in char_list)
    assert gt.dtype == np.int32 and gt_lens.dtype == np.int32 and gt.shape[0] == gt_lens.shape[0] == len(bounds) == len(texts)
    assert gt.shape[2] == S and gt.shape[1] == (int(gt_lens.max()) if len(texts) else 2)
    for b, text in enumerate(texts):
        want, want_bounds = cs.prepare_text(cs.CtcSegmentationParameters(char_list=list(char_list)), [text])
        n = want.shape[0]
        assert gt_lens[b] == n and list(bounds[b]) == list(want_bounds), (b, text)
        assert np.array_equal(gt[b, :n], want), (b, text)
        assert np.all(gt[b, n:] == -1), (b, text)
    return gt, gt_lens, bounds


def test_pack_empty_text_and_characters_outside_the_list():
    gt, gt_lens, bounds = check_pack(ABC, ["", "a?b.,c·xyz", "abc", "»«"])
    assert gt_lens.tolist() == [2, 6, 6, 2] and list(bounds[0]) == [1, 1] and list(bounds[1]) == [1, 5]      # "#·abc·"
    assert gt[0, 1, 0] == 0 and gt[0, 0, 0] == -1            # the separator is the blank token; '#' is no token


def test_pack_alphabet_with_multi_character_tokens():
    texts = ["".join(p) for n in range(1, 5) for p in itertools.product("abc", repeat=n)][::3] + ["abcabcab", "cabab"]
    gt, gt_lens, _ = check_pack(ABC, texts)
    row = texts.index("abcabcab")
    assert int((gt[row, :, 1:] >= 0).sum()) >= 5             # "ab" x 3 and "abc" x 2: real entries with s > 0
    assert int((gt[:, :, 1:] >= 0).sum()) >= 9


def test_pack_synthetic_token_list():
    toks = synthetic_token_list(96, 3)[:-1]
    rng = np.random.default_rng(0)
    body = [t for t in toks if len(t) == 1 and t not in cs.CtcSegmentationParameters.excluded_characters]
    texts = ["".join(rng.choice(body, size=n)) for n in (0, 1, 7, 45, 68)] + ["。、?!," + body[0] + " 　" + "Z"]
    gt, gt_lens, bounds = check_pack(toks, texts)
    assert gt.shape[2] == 7                                   # "<blank>"
    assert gt_lens.tolist()[:5] == [2, 4, 10, 48, 71]
    assert check_pack(toks, [])[0].shape == (0, 2, 7)


def test_pack_with_separators_inside_the_text():
    """replace_spaces_with_blanks puts separators between words: spans across them are looked up with the blank's text, as
    prepare_text does"""
    char_list = ["<blank>", "a", "b", "a<blank>", "<blank>b", "ab"]
    params = cs.CtcSegmentationParameters(char_list=char_list, replace_spaces_with_blanks=True)
    texts = ["ab a b", " a  b ", "ba"]
    gt, gt_lens, bounds = cs.pack_ground_truth(params, texts)
    for b, text in enumerate(texts):
        want, want_bounds = cs.prepare_text(cs.CtcSegmentationParameters(char_list=char_list, replace_spaces_with_blanks=True), [text])
        assert gt_lens[b] == want.shape[0] and list(bounds[b]) == list(want_bounds)
        assert np.array_equal(gt[b, :gt_lens[b]], want) and np.all(gt[b, gt_lens[b]:] == -1)
    assert int((gt[:, :, 1:] >= 0).sum()) >= 3


def test_header_declares_and_library_exports_the_aligner():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rs_asr.h")).read(), flags=re.S)
    assert re.search(r"\bsize_t\s+rs_ctc_align_workspace_bytes\s*\(\s*const\s+rs_ctx\s*\*\s*ctx\s*,\s*int\s+B\s*,\s*int\s+tp_max\s*,\s*int\s+c_max\s*,\s*int\s+S\s*\)", src)
    assert re.search(r"\bint\s+rs_ctc_align\s*\(\s*rs_ctx\s*\*\s*ctx\s*,\s*const\s+float\s*\*\s*probs\s*,\s*int\s+ld\s*,", src)
    assert re.search(r"#define\s+RS_ABI_VERSION\s+7\b", src)
    lib = ctypes.CDLL(rs_build.build())
    assert hasattr(lib, "rs_ctc_align") and hasattr(lib, "rs_ctc_align_workspace_bytes")
    assert lib.rs_abi_version() == 7
    assert "rs_ctc_align" in capi.EXPORTS and "rs_ctc_align_workspace_bytes" in capi.EXPORTS
    lib.rs_ctc_align_workspace_bytes.restype = ctypes.c_size_t
    lib.rs_ctc_align_workspace_bytes.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 4
    assert lib.rs_ctc_align_workspace_bytes(None, 4, 10, 5, 3) == 0            # no context: the query refuses, it does not crash
    lib.rs_ctc_align.argtypes = capi.load().rs_ctc_align.argtypes
    assert lib.rs_ctc_align(None, None, 4, None, 1, 4, None, None, 2, 1, 0, None, None, None, 0, None) == capi.RS_EINVAL


def test_load_model_refuses_an_unknown_segmentation_mode():
    etr = importlib.import_module("reazonspeech_amd.espnet.asr.transcribe")
    with pytest.raises(ValueError, match="segmentation"):
        etr.load_model(segmentation="bogus", synthetic=True)
