"""The float64 front-end references of tests/frontend_ref.py against what the project already trusts: each float32 oracle
(oracle.model.frontend, oracle.espnet.frontend, oracle.zipformer.fbank) and, for kind 0, the HF features committed in
tests/golden/parakeet_tiny.npz — each within the tolerance the existing test against that oracle or golden states (2e-3, 2e-3,
5e-3).  Plus the three frame-count formulas for every length 0 .. 700 and the number of reflections kaldi's window extraction needs."""
import os

import numpy as np
import pytest
import torch

import frontend_ref as fr
from oracle import espnet as oe, model as om, zipformer as oz
from reazonspeech_amd.runtime.config import ESPNET_TINY, TINY
from reazonspeech_amd.runtime.k2_config import ZIPFORMER_TINY
from reazonspeech_amd.runtime.weights import synthetic_state_dict
from reazonspeech_amd.runtime.weights_espnet import synthetic_state_dict_espnet

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "parakeet_tiny.npz")
LENGTHS = (8000, 17231, 30001, 48000)          # 0.5 .. 3 s
TOL_NEMO, TOL_ESPNET, TOL_KALDI = 2e-3, 2e-3, 5e-3


def noise(n, seed):
    return (0.1 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


@pytest.fixture(scope="module")
def sd_nemo():
    return synthetic_state_dict(TINY, 3)


@pytest.fixture(scope="module")
def sd_espnet():
    return synthetic_state_dict_espnet(ESPNET_TINY, 3)


@pytest.mark.parametrize("L", LENGTHS)
def test_nemo_reference_vs_float32_oracle(sd_nemo, L):
    x = noise(L, L)
    want, n = om.frontend(TINY, sd_nemo, torch.from_numpy(x)[None], torch.tensor([L]))
    got = fr.nemo_logmel(TINY, sd_nemo, x)
    assert got.shape == (int(n[0]), TINY.n_mels) == (L // 160, 80)
    assert np.abs(got - want[0].double().numpy()).max() <= TOL_NEMO


def test_nemo_reference_pads_like_pad_audio(sd_nemo):
    x = noise(9000, 1)
    padded = np.pad(x, (8000, 4000))
    assert np.array_equal(fr.nemo_logmel(TINY, sd_nemo, x, 8000, 4000), fr.nemo_logmel(TINY, sd_nemo, padded))
    want, _ = om.frontend(TINY, sd_nemo, torch.from_numpy(padded)[None], torch.tensor([len(padded)]))
    assert np.abs(fr.nemo_logmel(TINY, sd_nemo, x, 8000, 4000) - want[0].double().numpy()).max() <= TOL_NEMO


def test_nemo_reference_vs_hf_golden():
    gold = np.load(GOLD)
    sd = synthetic_state_dict(TINY, int(gold["seed"]), blank_bias=float(gold["blank_bias"]))
    for b, L in enumerate(gold["lengths"].tolist()):
        got = fr.nemo_logmel(TINY, sd, gold["audio"][b, :L])
        n = int(gold["hf_n_frames"][b])
        assert got.shape[0] == n
        assert np.abs(got - gold["hf_feats"][b, :n].astype(np.float64)).max() <= TOL_NEMO


def test_nemo_reference_one_frame_is_nan_and_no_frame_is_empty(sd_nemo):
    assert np.isnan(fr.nemo_logmel(TINY, sd_nemo, noise(160, 2))).all()
    assert fr.nemo_logmel(TINY, sd_nemo, noise(159, 2)).shape == (0, 80)


@pytest.mark.parametrize("L", LENGTHS)
def test_espnet_reference_vs_float32_oracle(sd_espnet, L):
    x = noise(L, L + 1)
    want, n = oe.frontend(ESPNET_TINY, sd_espnet, torch.from_numpy(x)[None], torch.tensor([L]))
    got = fr.espnet_logmel(ESPNET_TINY, sd_espnet, x)
    assert got.shape == (int(n[0]), 80) == (1 + L // 128, 80)
    assert np.abs(got - want[0].double().numpy()).max() <= TOL_ESPNET


def test_espnet_reference_refuses_what_torch_refuses(sd_espnet):
    with pytest.raises(ValueError):
        fr.espnet_logmel(ESPNET_TINY, sd_espnet, noise(256, 0))
    x = noise(257, 0)
    want, _ = oe.frontend(ESPNET_TINY, sd_espnet, torch.from_numpy(x)[None], torch.tensor([257]))
    assert np.abs(fr.espnet_logmel(ESPNET_TINY, sd_espnet, x) - want[0].double().numpy()).max() <= TOL_ESPNET


@pytest.mark.parametrize("L", LENGTHS + (80, 100, 241))
def test_kaldi_reference_vs_float32_oracle(L):
    x = noise(L, L + 2)
    want = oz.fbank(ZIPFORMER_TINY, torch.from_numpy(x))
    got = fr.kaldi_fbank(ZIPFORMER_TINY, x)
    assert got.shape == tuple(want.shape) == ((L + 80) // 160, 80)
    assert np.abs(got - want.double().numpy()).max() <= TOL_KALDI


def test_frame_counts_for_every_short_length(sd_nemo, sd_espnet):
    for L in range(701):
        x = noise(L, 7)
        assert fr.nemo_frames(L) == L // 160 == TINY.mel_frames(L) == fr.nemo_logmel(TINY, sd_nemo, x).shape[0]
        assert fr.espnet_frames(L) == 1 + L // 128 == ESPNET_TINY.mel_frames(L)
        if L > 256:
            assert fr.espnet_logmel(ESPNET_TINY, sd_espnet, x).shape[0] == 1 + L // 128
        assert fr.kaldi_frames(L) == (L + 80) // 160 == ZIPFORMER_TINY.fbank_frames(L) == fr.kaldi_fbank(ZIPFORMER_TINY, x).shape[0]


def test_kaldi_reflection_count():
    """a frame reaches at most 120 samples before the signal and, with n = (L + 80) // 160 frames, 160 (n - 1) + 279 - (L - 1) <= 200
    samples past it; a reflection brings an index that is d samples outside to d - 1 samples inside the same edge, i.e. d - L
    outside the other one: ceil(200 / L) reflections, 3 at L = 80 and never more for a longer signal"""
    assert [fr.kaldi_bounces(L) for L in (1, 79, 80, 81, 100, 200, 240, 400, 401)] == [0, 0, 3, 3, 2, 1, 1, 1, 1]
    assert max(fr.kaldi_bounces(L) for L in range(80, 701)) == 3
    idx, bounces = fr.kaldi_reflect(np.array([-1, -2, 5, 6, -7, 13]), 6)
    assert idx.tolist() == [0, 1, 5, 5, 5, 1] and bounces == 2
