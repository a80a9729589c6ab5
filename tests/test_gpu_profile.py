"""-m gpu: the profiling brackets (rs_profile_enable / _read / _read_launches / _reset; csrc/rs_common.h: rs_prof_scope).

A bracket is one (start, stop) event pair around the launches of one class plus host bookkeeping: the class's `launches`, `flops`
and `bytes` and one (M, N, K, flags, flops) record per bracket.  All of that is host arithmetic over shapes, so it is compared
EXACTLY; only the times depend on the run.

One "pass" per family (toy configurations, two synthetic utterances of 1.0 s and 0.6 s): front end, encoder, greedy search and
token scores (`run_device` with token_scores on), then the family's beam search on the same projection — nemo: ALSD 4, espnet:
the default beam search 4, k2: the modified beam search 4.

  profiling changes no result     the pass with no class enabled == the pass with all six: ids, frames, the bits of the token
                                  log-probabilities and of the beam scores
  brackets are counted as before  the counts and records of one profiled pass == PARENT, recorded by `record()` below on the
                                  commit before the scope guard (hand-balanced rs_prof_begin / rs_prof_end);
                                  rs_rnnt_greedy / _alsd / _beam / _mbs / _token_scores record exactly one DECODE bracket per call
  pairs stay in step              3 passes without a reset: 3 x the counts and the records, every time finite and >= 0; zero after
                                  a reset
  an error inside a bracket       rs_gemm_bf16 with a Swoosh activation and a row mask passes the launcher's argument checks and
                                  is refused (RS_EINVAL) by the tile dispatch, inside the open GEMM bracket and before any launch;
                                  afterwards the pairs are still in step.  (No other class has an error return inside a bracket
                                  that arguments alone reach: the rest are HIP failures or states a finalized context excludes.)
"""
import math

import numpy as np
import pytest
import torch

from reazonspeech_amd.espnet.asr.model import EspnetModel, synthetic_token_list
from reazonspeech_amd.k2.asr.model import K2Model, synthetic_tokens
from reazonspeech_amd.runtime import capi
from reazonspeech_amd.runtime.config import ESPNET_TINY, TINY
from reazonspeech_amd.runtime.k2_config import ZIPFORMER_TINY
from reazonspeech_amd.runtime.k2_weights import synthetic_state_dict_k2
from reazonspeech_amd.runtime.model import AsrModel
from reazonspeech_amd.runtime.synth import synthetic_batch
from reazonspeech_amd.runtime.tokenizer import SyntheticTokenizer
from reazonspeech_amd.runtime.weights import synthetic_state_dict
from reazonspeech_amd.runtime.weights_espnet import synthetic_state_dict_espnet

pytestmark = pytest.mark.gpu
FAMILIES = ("nemo", "espnet", "k2")
CLASSES = {"gemm": capi.PROF_GEMM, "attention": capi.PROF_ATTN, "frontend": capi.PROF_FRONTEND, "decode": capi.PROF_DECODE,
           "elementwise": capi.PROF_ELEMENTWISE, "subsample": capi.PROF_SUBSAMPLE}
ALL = sum(CLASSES.values())

# PARENT[family] = (counts, records) of one profiled pass, as `profile(ctx)` returns them: counts[class] = [launches, flops, bytes],
# records[class] = [[M, N, K, flags, flops], ..] in launch order.  Recorded on an MI355X with `record()` at commit d70a71a.
PARENT = {'espnet': ({'attention': [2, 5529600.0, 245760.0],
             'decode': [3, 0.0, 0.0],
             'elementwise': [12, 2641920.0, 1075200.0],
             'frontend': [1, 6302772.0, 370944.0],
             'gemm': [19, 1734082560.0, 16300032.0],
             'subsample': [1, 22284288.0, 2556672.0]},
            {'attention': [[0, 0, 0, 0, 2764800.0], [0, 0, 0, 0, 2764800.0]],
             'decode': [[0, 0, 0, 0, 0.0], [0, 0, 0, 0, 0.0], [0, 0, 0, 0, 0.0]],
             'elementwise': [[0, 0, 0, 0, 122880.0], [0, 0, 0, 0, 122880.0], [0, 0, 0, 0, 122880.0], [0, 0, 0, 0, 645120.0],
                             [0, 0, 0, 0, 122880.0], [0, 0, 0, 0, 245760.0], [0, 0, 0, 0, 122880.0], [0, 0, 0, 0, 122880.0],
                             [0, 0, 0, 0, 645120.0], [0, 0, 0, 0, 122880.0], [0, 0, 0, 0, 122880.0], [0, 0, 0, 0, 122880.0]],
             'frontend': [[0, 0, 0, 0, 6302772.0]],
             'gemm': [[1140, 256, 2304, 35, 1344798720.0], [60, 256, 4864, 17, 149422080.0], [60, 512, 256, 5, 15728640.0],
                      [60, 256, 512, 25, 15728640.0], [60, 768, 256, 1, 23592960.0], [60, 256, 256, 25, 7864320.0],
                      [60, 512, 256, 65, 15728640.0], [60, 256, 256, 25, 7864320.0], [60, 512, 256, 5, 15728640.0],
                      [60, 256, 512, 25, 15728640.0], [60, 512, 256, 5, 15728640.0], [60, 256, 512, 25, 15728640.0],
                      [60, 768, 256, 1, 23592960.0], [60, 256, 256, 25, 7864320.0], [60, 512, 256, 65, 15728640.0],
                      [60, 256, 256, 25, 7864320.0], [60, 512, 256, 5, 15728640.0], [60, 256, 512, 25, 15728640.0],
                      [60, 128, 256, 17, 3932160.0]],
             'subsample': [[0, 0, 0, 0, 22284288.0]]}),
 'k2': ({'attention': [16, 4761088.0, 169728.0],
         'decode': [3, 0.0, 0.0],
         'elementwise': [8, 1235968.0, 153600.0],
         'frontend': [1, 5002200.0, 320000.0],
         'gemm': [73, 256675840.0, 9051328.0],
         'subsample': [2, 0.0, 0.0]},
        {'attention': [[0, 0, 0, 0, 1354240.0], [0, 0, 0, 0, 406272.0], [0, 0, 0, 0, 270848.0], [0, 0, 0, 0, 270848.0],
                       [0, 0, 0, 0, 677120.0], [0, 0, 0, 0, 203136.0], [0, 0, 0, 0, 135424.0], [0, 0, 0, 0, 135424.0],
                       [0, 0, 0, 0, 677120.0], [0, 0, 0, 0, 203136.0], [0, 0, 0, 0, 135424.0], [0, 0, 0, 0, 135424.0],
                       [0, 0, 0, 0, 92160.0], [0, 0, 0, 0, 27648.0], [0, 0, 0, 0, 18432.0], [0, 0, 0, 0, 18432.0]],
         'decode': [[0, 0, 0, 0, 0.0], [0, 0, 0, 0, 0.0], [0, 0, 0, 0, 0.0]],
         'elementwise': [[0, 0, 0, 0, 247296.0], [0, 0, 0, 0, 247296.0], [0, 0, 0, 0, 153088.0], [0, 0, 0, 0, 153088.0],
                         [0, 0, 0, 0, 153088.0], [0, 0, 0, 0, 153088.0], [0, 0, 0, 0, 64512.0], [0, 0, 0, 0, 64512.0]],
         'frontend': [[0, 0, 0, 0, 5002200.0]],
         'gemm': [[1748, 64, 192, 273, 42958848.0], [1748, 192, 64, 129, 42958848.0], [1748, 64, 192, 25, 42958848.0],
                  [92, 64, 1216, 17, 14319616.0], [92, 136, 64, 1, 1601536.0], [92, 192, 64, 129, 2260992.0],
                  [92, 64, 192, 25, 2260992.0], [92, 144, 64, 1, 1695744.0], [92, 64, 64, 25, 753664.0],
                  [92, 24, 64, 1, 282624.0], [92, 64, 64, 25, 753664.0], [92, 128, 64, 65, 1507328.0],
                  [92, 64, 64, 25, 753664.0], [92, 256, 64, 129, 3014656.0], [92, 64, 256, 25, 3014656.0],
                  [92, 24, 64, 1, 282624.0], [92, 64, 64, 25, 753664.0], [92, 128, 64, 65, 1507328.0],
                  [92, 64, 64, 25, 753664.0], [92, 320, 64, 129, 3768320.0], [92, 64, 320, 25, 3768320.0],
                  [46, 272, 128, 1, 3203072.0], [46, 192, 128, 129, 2260992.0], [46, 128, 192, 25, 2260992.0],
                  [46, 288, 128, 1, 3391488.0], [46, 128, 128, 25, 1507328.0], [46, 48, 128, 1, 565248.0],
                  [46, 128, 64, 25, 753664.0], [46, 256, 128, 65, 3014656.0], [46, 128, 128, 25, 1507328.0],
                  [46, 256, 128, 129, 3014656.0], [46, 128, 256, 25, 3014656.0], [46, 48, 128, 1, 565248.0],
                  [46, 128, 64, 25, 753664.0], [46, 256, 128, 65, 3014656.0], [46, 128, 128, 25, 1507328.0],
                  [46, 320, 128, 129, 3768320.0], [46, 128, 320, 25, 3768320.0], [46, 272, 128, 1, 3203072.0],
                  [46, 192, 128, 129, 2260992.0], [46, 128, 192, 25, 2260992.0], [46, 288, 128, 1, 3391488.0],
                  [46, 128, 128, 25, 1507328.0], [46, 48, 128, 1, 565248.0], [46, 128, 64, 25, 753664.0],
                  [46, 256, 128, 65, 3014656.0], [46, 128, 128, 25, 1507328.0], [46, 256, 128, 129, 3014656.0],
                  [46, 128, 256, 25, 3014656.0], [46, 48, 128, 1, 565248.0], [46, 128, 64, 25, 753664.0],
                  [46, 256, 128, 65, 3014656.0], [46, 128, 128, 25, 1507328.0], [46, 320, 128, 129, 3768320.0],
                  [46, 128, 320, 25, 3768320.0], [24, 136, 64, 1, 417792.0], [24, 192, 64, 129, 589824.0],
                  [24, 64, 192, 25, 589824.0], [24, 144, 64, 1, 442368.0], [24, 64, 64, 25, 196608.0], [24, 24, 64, 1, 73728.0],
                  [24, 64, 64, 25, 196608.0], [24, 128, 64, 65, 393216.0], [24, 64, 64, 25, 196608.0],
                  [24, 256, 64, 129, 786432.0], [24, 64, 256, 25, 786432.0], [24, 24, 64, 1, 73728.0],
                  [24, 64, 64, 25, 196608.0], [24, 128, 64, 65, 393216.0], [24, 64, 64, 25, 196608.0],
                  [24, 320, 64, 129, 983040.0], [24, 64, 320, 25, 983040.0], [46, 128, 128, 17, 1507328.0]],
         'subsample': [[0, 0, 0, 0, 0.0], [0, 0, 0, 0, 0.0]]}),
 'nemo': ({'attention': [2, 3840000.0, 204800.0],
           'decode': [3, 0.0, 0.0],
           'elementwise': [11, 1792000.0, 793600.0],
           'frontend': [1, 10004400.0, 640000.0],
           'gemm': [20, 236748800.0, 6888960.0],
           'subsample': [2, 16704000.0, 704000.0]},
          {'attention': [[0, 0, 0, 0, 1920000.0], [0, 0, 0, 0, 1920000.0]],
           'decode': [[0, 0, 0, 0, 0.0], [0, 0, 0, 0, 0.0], [0, 0, 0, 0, 0.0]],
           'elementwise': [[0, 0, 0, 0, 102400.0], [0, 0, 0, 0, 102400.0], [0, 0, 0, 0, 102400.0], [0, 0, 0, 0, 384000.0],
                           [0, 0, 0, 0, 102400.0], [0, 0, 0, 0, 204800.0], [0, 0, 0, 0, 102400.0], [0, 0, 0, 0, 102400.0],
                           [0, 0, 0, 0, 384000.0], [0, 0, 0, 0, 102400.0], [0, 0, 0, 0, 102400.0]],
           'frontend': [[0, 0, 0, 0, 10004400.0]],
           'gemm': [[2000, 64, 64, 35, 16384000.0], [500, 64, 64, 35, 4096000.0], [50, 256, 640, 17, 16384000.0],
                    [50, 512, 256, 5, 13107200.0], [50, 256, 512, 25, 13107200.0], [50, 768, 256, 1, 19660800.0],
                    [50, 256, 256, 25, 6553600.0], [50, 512, 256, 65, 13107200.0], [50, 256, 256, 25, 6553600.0],
                    [50, 512, 256, 5, 13107200.0], [50, 256, 512, 25, 13107200.0], [50, 512, 256, 5, 13107200.0],
                    [50, 256, 512, 25, 13107200.0], [50, 768, 256, 1, 19660800.0], [50, 256, 256, 25, 6553600.0],
                    [50, 512, 256, 65, 13107200.0], [50, 256, 256, 25, 6553600.0], [50, 512, 256, 5, 13107200.0],
                    [50, 256, 512, 25, 13107200.0], [50, 128, 256, 17, 3276800.0]],
           'subsample': [[0, 0, 0, 0, 16128000.0], [0, 0, 0, 0, 576000.0]]})}

_scenes = {}


def scene(family):
    """per family, once: the runtime model (token scores on; the weight recipes of tests/test_gpu_token_scores.py, on which the
    searches emit tokens and the espnet beam search stays within its bound) and the ragged batch staged on the device"""
    if family not in _scenes:
        kw = dict(device="cuda:0", token_scores=True)
        if family == "nemo":
            am = AsrModel(TINY, synthetic_state_dict(TINY, 0, blank_bias=3.5, dec_gain=4.0), SyntheticTokenizer(TINY.vocab_size), **kw)
        elif family == "espnet":
            sd = synthetic_state_dict_espnet(ESPNET_TINY, 11, blank_bias=12.0, dec_gain=8.0)
            am = EspnetModel(ESPNET_TINY, sd, synthetic_token_list(ESPNET_TINY.vocab_size, 11), **kw).am
        else:
            am = K2Model(ZIPFORMER_TINY, synthetic_state_dict_k2(ZIPFORMER_TINY, 3), synthetic_tokens(ZIPFORMER_TINY.vocab_size, 3), **kw).am
        audio, _ = synthetic_batch(2, 1.0, seed=21)
        waves = [np.ascontiguousarray(audio[0, :16000]), np.ascontiguousarray(audio[1, :9600])]
        buf = am.stage(waves, buf=am.new_buffers(2, 16000))
        _scenes[family] = (am, buf)
    return _scenes[family]


def beam_search(family, am, buf):
    """the family's beam search through the C ABI on the projection `run_device` left -> (ids, frames, the scores' bytes)"""
    B, Tp = buf.B, buf.tp_max
    dev, stream = am.device, torch.cuda.current_stream().cuda_stream
    z = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)       # noqa: E731
    scores, n_ids = torch.zeros((B,), device=dev), z(B)
    if family == "nemo":
        ids, fr = z(B, 2 * Tp), z(B, 2 * Tp)
        ws = torch.empty((am.ctx.alsd_workspace_bytes(B, 4, Tp, 1.0),), dtype=torch.uint8, device=dev)
        am.ctx.rnnt_alsd(buf.joint_enc, buf.enc_lens, B, Tp, 4, 1.0, True, False, ids, fr, n_ids, scores, ws, stream)
    elif family == "espnet":
        ids, fr, pops = z(B, 2 * Tp + 16), z(B, 2 * Tp + 16), z(B)
        ws = torch.empty((am.ctx.beam_workspace_bytes(B, 4, Tp, 0),), dtype=torch.uint8, device=dev)
        am.ctx.rnnt_beam(buf.joint_enc, buf.enc_lens, B, Tp, 4, True, 0, ids, n_ids, scores, pops, ws, stream, frames=fr)
    else:
        ids, fr = z(B, Tp), z(B, Tp)
        ws = torch.empty((am.ctx.mbs_workspace_bytes(B, 4, Tp, Tp),), dtype=torch.uint8, device=dev)
        am.ctx.rnnt_mbs(buf.joint_enc, buf.enc_lens, B, Tp, 4, 0.0, True, ids, fr, n_ids, scores, ws, stream)
    torch.cuda.synchronize()
    n, ids, fr = n_ids.cpu().numpy(), ids.cpu().numpy(), fr.cpu().numpy()
    return [ids[b, :n[b]].tolist() for b in range(B)], [fr[b, :n[b]].tolist() for b in range(B)], scores.cpu().numpy().tobytes()


def one_pass(family, am, buf):
    """-> everything the pass computes: greedy ids and frames, the bits of their log-probabilities, the beam search's result"""
    am.run_device(buf)
    torch.cuda.synchronize()
    res = am.collect(buf)
    return res.ids, res.frames, [np.asarray(x, np.float32).tobytes() for x in res.token_logprobs], beam_search(family, am, buf)


def profile(ctx):
    """-> (counts[class] = [launches, flops, bytes], records[class] = [[M, N, K, flags, flops], ..], every record's time)"""
    counts, records, ms = {}, {}, []
    for name, klass in CLASSES.items():
        r = ctx.profile_read(klass)
        counts[name] = [r["launches"], r["flops"], r["bytes"]]
        launches = ctx.profile_launches(klass)
        records[name] = [list(rec[:5]) for rec in launches]
        ms += [rec[5] for rec in launches]
    return counts, records, ms


def profiled_passes(family, n):
    """n passes with all six classes enabled -> ([the passes' results], profile(ctx)).  One more profiled pass runs first, before
    the reset: a GEMM launched while its class is off leaves its (M, N, K, flags) tag behind for the first bracket that is
    recorded later, whichever class that is, so the first record after enabling depends on what the context ran before."""
    am, buf = scene(family)
    am.ctx.profile_enable(ALL)
    try:
        one_pass(family, am, buf)
        am.ctx.profile_reset()
        results = [one_pass(family, am, buf) for _ in range(n)]
        return results, profile(am.ctx)
    finally:
        am.ctx.profile_enable(0)


_single = {}


def single(family):
    """the results and the profile of one profiled pass (shared: computed once per family)"""
    if family not in _single:
        results, prof = profiled_passes(family, 1)
        _single[family] = (results[0], prof)
    return _single[family]


def record():
    """prints the PARENT table (run once on the commit the counts are to be compared with)"""
    import pprint
    print("PARENT = " + pprint.pformat({family: single(family)[1][:2] for family in FAMILIES}, width=128, compact=True))


def check_in_step(family, n, one):
    """n passes without a reset: n x the counts and the records of one pass, times finite and >= 0; a reset clears everything"""
    am, _ = scene(family)
    _, (counts, records, ms) = profiled_passes(family, n)
    for name in CLASSES:
        assert counts[name] == [n * one[0][name][0], n * one[0][name][1], n * one[0][name][2]], (family, name)
        assert records[name] == n * one[1][name], (family, name)
        assert len(records[name]) == counts[name][0]
    assert len(ms) == sum(c[0] for c in counts.values()) and all(math.isfinite(t) and t >= 0.0 for t in ms), (family, ms)
    am.ctx.profile_reset()
    counts, records, ms = profile(am.ctx)
    assert all(c == [0, 0.0, 0.0] for c in counts.values()) and not any(records.values()) and not ms


@pytest.mark.parametrize("family", FAMILIES)
def test_profiling_changes_no_result(gpu_device, family):
    am, buf = scene(family)
    am.ctx.profile_enable(0)
    plain = one_pass(family, am, buf)
    assert profile(am.ctx)[0] == {name: [0, 0.0, 0.0] for name in CLASSES}, "nothing is recorded with no class enabled"
    print(f"{family}: enc_lens {buf.enc_lens.tolist()}, greedy tokens {[len(x) for x in plain[0]]}, beam tokens {[len(x) for x in plain[3][0]]}")
    assert sum(len(x) for x in plain[0]) > 0 and sum(len(x) for x in plain[3][0]) > 0, "re-choose the inputs: the searches must emit tokens"
    assert single(family)[0] == plain


@pytest.mark.parametrize("family", FAMILIES)
def test_brackets_are_counted_as_before(gpu_device, family):
    counts, records, _ = single(family)[1]
    assert counts == PARENT[family][0]
    assert records == PARENT[family][1]
    # every search and the scoring pass is one DECODE bracket, whatever it launches inside
    am, buf = scene(family)
    stream = torch.cuda.current_stream().cuda_stream
    calls = {"greedy": lambda: am.decode(am.ctx, buf, buf.ws, stream), "token_scores": lambda: am.score(am.ctx, buf, stream),
             {"nemo": "alsd", "espnet": "beam", "k2": "mbs"}[family]: lambda: beam_search(family, am, buf)}
    am.ctx.profile_enable(ALL)
    try:
        for what, call in calls.items():
            am.ctx.profile_reset()
            call()
            torch.cuda.synchronize()
            got = {name: c[0] for name, c in profile(am.ctx)[0].items()}
            assert got == {name: int(name == "decode") for name in CLASSES}, (family, what, got)
    finally:
        am.ctx.profile_enable(0)
        am.ctx.profile_reset()


@pytest.mark.parametrize("family", FAMILIES)
def test_pairs_stay_in_step(gpu_device, family):
    check_in_step(family, 3, single(family)[1])


@pytest.mark.parametrize("family", FAMILIES)
def test_pairs_stay_in_step_after_an_error_inside_a_bracket(gpu_device, family):
    am, _ = scene(family)
    A = torch.zeros((64, 64), dtype=torch.bfloat16, device=am.device)
    W, out = torch.zeros((64, 64), dtype=torch.bfloat16, device=am.device), torch.zeros((64, 64), dtype=torch.bfloat16, device=am.device)
    lens = torch.full((1,), 64, dtype=torch.int32, device=am.device)
    am.ctx.profile_enable(ALL)
    am.ctx.profile_reset()
    with pytest.raises(capi.RsError, match="row mask") as e:
        am.ctx.gemm(A, W, out, flags=capi.GEMM_SWOOSHL | capi.GEMM_ROWMASK, mask_lens=lens, mask_rows=64, mask_steps=1,
                    stream=torch.cuda.current_stream().cuda_stream)
    assert e.value.code == capi.RS_EINVAL
    torch.cuda.synchronize()
    counts, records, ms = profile(am.ctx)                  # the refused call is one closed bracket: begun, ended, nothing launched
    assert counts["gemm"][0] == 1 and records["gemm"] == [[64, 64, 64, capi.GEMM_SWOOSHL | capi.GEMM_ROWMASK, 2.0 * 64 * 64 * 64]]
    assert len(ms) == 1 and math.isfinite(ms[0]) and ms[0] >= 0.0
    check_in_step(family, 3, single(family)[1])
