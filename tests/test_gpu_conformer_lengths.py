"""-m gpu: the two Conformer encoders as WHOLE MODELS at the utterance lengths that pick each kernel form (toy geometries;
rs_encoder_forward / rs_encoder_forward_f32 of csrc/k_conformer.hip).  Fixtures, oracles and the comparison: tests/conformer_lengths_ref.py;
tests/test_conformer_lengths_host.py checks them on the CPU (sample counts, decision margins, a mutated oracle is caught).

  nemo    TINY: 2 layers, d_model 256, 2 heads of 128 (the 619M model's head width), conv kernel 9, dw_striding x8
  espnet  ESPNET_TINY: 2 layers, d_model 256, 4 heads of 64 (the 120M model's head width), conv kernel 15, Conv2dSubsampling x4
  nemo_w  TINY with att_left 20, att_right 10, one global token (section 4)
Every model is an AsrModel with pad_seconds = 0; an utterance of T' frames is `runtime/synth.py` audio of `samples_for(cfg, T')` samples.

The encoder chooses its kernels from the frame count T' of the BUFFER (qb = ceil(T' / 32) query / key blocks):
  launch_attention_hd<128>            min(qb, 6) waves per workgroup, ceil(qb / 6) workgroups per head; keys staged KB_CHUNK = 5 blocks at a time
  launch_attention_hd<64>             T' <= 32: one wave, relpos_attention_kernel<64,0,0,2>; above: <64,0,0,4>, min(qb, 4) waves, chunks of 4 key blocks
  WINDOW (bf16, nemo_w)               relpos_attention_kernel<128,0,1>, the geometry of the first row
  rs_launch_attention_f32             full attention: attention_f32_mfma_kernel, 64-query grids; windowed: attention_f32_keys_kernel<4> for
                                      T' <= 256, <8> for T' <= 512, <0> above (scores computed twice; one body, the same bits from all three)
  conv module, fuse_glu = 1           k = 9: dwconv_silu_dma_kernel<9,6>, 48-frame tiles; k = 15: dwconv_act_kernel<15,0>, 128-frame tiles
  conv module, fuse_glu = 0           k = 9: glu_dwconv_silu_fast_kernel<9,6,1>, 48-frame tiles; k = 15: glu_dwconv_silu_kernel, 32-frame tiles
  float32 conv module                 glu_dwconv_silu_f32_kernel: one thread per output, no forms
  positions                           rows (tcap - T') .. of pos.table / L.pos_proj (bf16) or pos.table.f32 (projected per call), npos = 2 T' - 1
  output LayerNorm                    without a tap on the layer it is DEFERRED: layernorm2 leaves (mean, rstd) and the next layer's first
                                      residual GEMM normalises its residual operand (res_ln); with a tap the rows are written.  Every
                                      ladder case runs both ways: untapped first (enc, joint, ids against the oracle), then with the taps, and
                                      the two runs must agree bit for bit

1. LENGTH LADDER, float32 and bf16 mode, each utterance alone in a buffer sized to it.  T' -> form (`forms()` of the helper prints it):
   nemo    1 2 3 4 5 8 9     one wave, one key block, M = T' rows (M = 1, npos = 1 at T' = 1); shorter than the depthwise half-width 4 up to
                             T' = 4, above it from 5; float32 MFMA: one partly filled 64-query grid
           31 32 33          1 / 1 / 2 waves and key blocks
           47 48 49          one 48-frame conv tile / one / two
           63 64 65          2 / 2 / 3 waves; the float32 MFMA 64-query grid: 1 / 1 / 2
           95 96 97          3 / 3 / 4 waves; two conv tiles / two / three
           159 160 161       5 / 5 / 6 waves; ONE key chunk of 5 blocks / one / two chunks
           191 192 193       6 waves in one workgroup / the same / 7 blocks: a second workgroup of 6 waves with one block of queries
           319 320 321       two key chunks / two / three; two workgroups
           385               13 blocks: three workgroups, three key chunks; 9 conv tiles; 7 float32 grids
   espnet  1 2 3 7 8 9       one wave <.,2>; shorter than the depthwise half-width 7 up to T' = 7
           31 32 33          <.,2> one wave / <.,2> / <.,4> two waves; the 32-frame tile of the unfused conv kernel
           63 64 65          <.,4> 2 / 2 / 3 waves; float32 grids 1 / 1 / 2
           127 128 129       4 waves in ONE workgroup, ONE chunk of 4 key blocks, ONE 128-frame depthwise tile / the same / a second
                             workgroup, a second chunk and a second tile together
           255 256 257       two workgroups and chunks / two / three
           383 384 385       three / three / four
           513               17 blocks: five workgroups, five chunks, five depthwise tiles, nine float32 grids
   float32 mode: sub_out, layer0, layer1, enc, joint (and the ESPnet CTC posteriors) within the family's float32 tolerance (TOL_ENC of
   tests/test_gpu_fp32_mode.py, TOL_F32 of tests/test_gpu_espnet_fp32.py: 1e-4) of the `fp32` oracle, enc_lens equal, ids and frames
   IDENTICAL to the oracle's own greedy search.  bf16 mode: the same taps within max 6e-2 / mean 6e-3 of the `bf16-fused-glu` recipe,
   CTC posteriors within 3e-2, ids and frames bit-exact against oracle/rnnt_greedy.c on the device's own projection.  Both: the LAST
   valid row on its own against the max tolerance; every row of enc and joint at and past the length finite.
   sub_out is the one tap that is not LayerNorm-ed (values up to 80: 1e-4 is 13 float32 ulps of them, 6e-2 an eighth of a bf16 ulp), and
   it sits right behind the log-mel front-end, whose float32 error (the logarithm of small bin powers) reaches it unnormalised.  Its
   bound is the larger of the tolerance above and the reference-only yardstick of tests/test_gpu_subsample_edges.py, taken over front-end
   and subsampling (`sub_out_yardstick`): float32 max(8 |oracle32 - oracle64|, 4 * 2^-23 max |oracle64|), bf16 max / mean |bf16 recipe
   - oracle32| with factor 1; both are printed beside the measured error.  Measured on an MI355X (worst of the ladders and section 4):
       float32  sub_out 1.36e-3 at espnet T' = 383 (bound 6.4e-3: the oracle's own float32 front-end is 2.0e-4 from float64 there, ten
                times its usual error) and 8.9e-4 at T' = 513 (bound 4.5e-3); every other case <= 2.1e-4 (bounds 1.0e-4 .. 1.1e-3), the
                closest 0.86 of its bound (espnet T' = 9: 9.9e-5 against 1.16e-4);
                layer0 / layer1 / enc / joint <= 5.2e-5, CTC 2.2e-6 (tolerance 1e-4)
       bf16     sub_out max 0.072 (bound 0.285), mean 5.5e-3 (bound 2.7e-2); layer0 / layer1 / enc max <= 8.1e-3, mean <= 1.1e-3, joint
                max 1.3e-2, mean 1.9e-3 (tolerance 6e-2 / 6e-3); CTC 2.8e-3 (3e-2); fuse_glu = 0 the same class (enc 6.6e-3, joint 1.0e-2)
2. THE OTHER CONV LAYOUT: fuse_glu = 0 (set_option, restored in a finally), bf16 only, T' = 3 32 33 48 49 129, both families, against the
   `bf16` recipe (pw1 stored bf16, GLU in the depthwise kernel).
3. ONE UTTERANCE THROUGH EVERY BUFFER LENGTH, bits, both modes, both families: T' = 9 33 129 161 193 alone, then as row 0 of buffers whose
   T' is 33 / 161 / 193 / 385 beside a full-length row, then all five in one ragged batch: encoder rows up to the length, joint
   projection, ids and frames `torch.equal` to the alone run.
4. LIMITED-CONTEXT ATTENTION (nemo_w): T' = 31 33 255 256 257 511 512 513; float32 through keys<4> / keys<8> / keys<0>, bf16 through
   the WINDOW kernel; the assertions of section 1 against the oracle with the same window; the T' = 257 utterance alone == inside the
   513-frame buffer, bits (keys<8> against keys<0> in float32: this rung showed that the one-wave-per-key-sum kernel, which ran
   above 512 frames before, changed an utterance's last bits with the buffer it rode in).
5. POSITION-TABLE CAPACITY, both modes, both families: a model built with pos_cap = 32 against the default on T' = 20, 200 (grows the
   tables to 256 through AsrModel.ensure_pos_cap), 20 again: bits equal between the models, and the first run == the third.
6. A ROW WITH NO OUTPUT FRAME inside a ragged batch (nemo: 128 samples, no feature frame; espnet: 704 samples = 6 feature frames, one too few
   for Conv2dSubsampling): it returns no ids, its encoder rows are finite, and its neighbours keep the bits of section 3.  Read
   beforehand, for both modes: enc_lens_kernel clamps the length to 0; the subsampling GEMMs' row masks zero every row of the utterance;
   the LayerNorms and GEMMs work on all B * T' rows whatever the lengths (a zero row normalises to beta: finite); relpos_attention_kernel,
   attention_f32_mfma_kernel and the keys kernels take len = min(lens[b], T'), visit no key block and write zeros for every query at or past
   it (asserted per operator with a length of 0 in tests/test_gpu_attention_edges.py); the depthwise kernels multiply the gated input by
   (t < len) and so convolve zeros (tests/test_gpu_convmod_ops.py, lengths 0 and 1); rnnt_init_kernel leaves a row with enc_len 0 off the
   alive list (tests/test_gpu_pipeline.py, lens[B // 2] = 0).  A whole BUFFER without an output frame (ESPnet, t_max = 6) is refused with
   RS_EINVAL by both modes' `Tp <= 0` check; the NeMo subsampling gives ceil(t_max / 8) >= 1 frames for every buffer rs_encoder_forward
   does not return early on (t_max = 0 is a no-op), so there is no such buffer to refuse.
7. THE PUBLIC PATH per family, both modes: `transcribe_batch` of three utterances == `transcribe` of each alone (text, subwords / segments, times).
   After the package's own padding (nemo 0.5 s each side, espnet 1 s + 0.5 s) the three have T' = 20 / 100 / 250 (nemo: 1, 4 and 6 + 2 waves)
   and T' = 50 / 200 / 450 (espnet: one, two and four workgroups).

Every case prints its worst error per tap; the worst per section lands in the suite's parity report beside espnet_parity's entries (keys
conformer_lengths_fp32 / conformer_lengths_bf16) and DESIGN.md keeps the figures beside the tolerances.
"""
import importlib

import numpy as np
import pytest
import torch

import conformer_lengths_ref as cl
from oracle import greedy as og
from reazonspeech_amd.runtime import capi
from reazonspeech_amd.runtime.model import AsrModel
from reazonspeech_amd.runtime.synth import synthetic_batch
from reazonspeech_amd.runtime.tokenizer import SyntheticTokenizer
from test_gpu_espnet_fp32 import TOL_F32 as TOL_ENC_ESPNET, report
from test_gpu_fp32_mode import TOL_ENC

pytestmark = pytest.mark.gpu
CFGS = cl.CFGS
TOL_FP32 = {"nemo": TOL_ENC, "nemo_w": TOL_ENC, "espnet": TOL_ENC_ESPNET}
LADDER_CASES = [(fam, t) for fam in ("nemo", "espnet") for t in cl.LADDER[fam]]
UNFUSED_CASES = [(fam, t) for fam in ("nemo", "espnet") for t in cl.UNFUSED_TP]
WINDOW_CASES = [("nemo_w", t) for t in cl.WINDOW_TP]
WORST = {"fp32": {}, "bf16": {}}


@pytest.fixture(scope="module")
def models(gpu_device):
    cache = {}

    def get(fam, precision, **kw):
        key = (fam, precision, tuple(sorted(kw.items())))
        if key not in cache:
            cache[key] = AsrModel(CFGS[fam], cl.weights(fam), None, device="cuda:0", pad_seconds=0.0, precision=precision, **kw)
        return cache[key]
    yield get
    cache.clear()
    ALONE.clear()
    torch.cuda.empty_cache()


class Run:
    """one pass of front-end, encoder and greedy search over `waves` in a buffer of `l_max` samples (default: the longest utterance)"""

    def __init__(self, model, waves, l_max=None, taps=False, ctc=False):
        cfg, dev = model.cfg, model.device
        l_max = max(int(l_max or 0), max(len(w) for w in waves))
        buf = model.stage(waves, l_max=l_max)
        B, tp, d = buf.B, buf.tp_max, cfg.d_model
        M = B * tp
        nan = float("nan")
        enc = torch.full((B, tp, d), nan, dtype=torch.float32, device=dev)
        buf.joint_enc.fill_(nan)
        sub = torch.full((M, d), nan, dtype=torch.float32, device=dev) if taps else None
        lay = torch.full((2, M, d), nan, dtype=torch.float32, device=dev) if taps else None
        vp = (cfg.n_logits + 3) // 4 * 4
        probs = torch.zeros((M, vp), dtype=torch.float32, device=dev) if ctc else None
        if taps:
            model.ctx.set_taps(sub, lay, (0, 1))
        if ctc:
            model.ctx.set_ctc_out(probs, None)
        try:
            model.run_device(buf, want_enc=enc)
            torch.cuda.synchronize()
        finally:
            model.ctx.set_taps()
            if ctc:
                model.ctx.set_ctc_out(None, None)
        self.buf, self.tp_max, self.got = buf, tp, model.collect(buf)
        self.enc, self.joint = enc.cpu(), buf.joint_enc.cpu()
        self.sub = sub.cpu().view(B, tp, d) if taps else None
        self.lay = lay.cpu().view(2, B, tp, d) if taps else None
        self.ctc = probs.cpu().view(B, tp, vp)[:, :, :cfg.n_logits] if ctc else None
        assert torch.isfinite(self.enc).all() and torch.isfinite(self.joint).all(), "a row at or past a length is not finite (or was not written)"

    def taps_of(self, b):
        n = self.got.enc_lens[b]
        out = {"enc": self.enc[b, :n], "joint": self.joint[b, :n]}
        if self.sub is not None:
            out.update({"sub_out": self.sub[b, :n], "layer0": self.lay[0, b, :n], "layer1": self.lay[1, b, :n]})
        if self.ctc is not None:
            out["ctc"] = self.ctc[b, :n]
        return out

    def outputs(self, b):
        n = self.got.enc_lens[b]
        return n, self.enc[b, :n].clone(), self.joint[b, :n].clone(), self.got.ids[b], self.got.frames[b]


def same_bits(a, b):
    return a[0] == b[0] and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and a[3] == b[3] and a[4] == b[4]


def note(mode, section, fam, tp, errs):
    w = WORST[mode].setdefault(section, {})
    for name, (mx, _, _) in errs.items():
        if mx > w.get(name, (-1.0,))[0]:
            w[name] = (mx, f"{fam}:{tp}")
    report("conformer_lengths_" + mode, {s: {k: {"max_err": v[0], "at": v[1]} for k, v in sorted(t.items())} for s, t in sorted(WORST[mode].items())})


def tapped_and_untapped(model, fam, tp):
    """the utterance alone, untapped (the deferred output LayerNorm) and with the taps: the two must agree bit for bit -> the tapped Run"""
    cfg = CFGS[fam]
    plain = Run(model, [cl.wave(fam, tp)])
    full = Run(model, [cl.wave(fam, tp)], taps=True, ctc=cfg.espnet)
    assert plain.tp_max == full.tp_max == tp, "the buffer is not sized to the utterance"
    assert same_bits(plain.outputs(0), full.outputs(0)), (fam, tp, "the tapped run differs from the untapped one")
    return full


def check_fp32(models, section, fam, tp):
    cfg = CFGS[fam]
    ref = cl.oracle(fam, tp, "fp32")
    run = tapped_and_untapped(models(fam, "fp32"), fam, tp)
    assert run.got.enc_lens == [ref["enc_len"]] == [tp]
    assert int(run.buf.n_frames[0]) == ref["n_frames"]
    names = cl.TAPS + (("ctc",) if cfg.espnet else ())
    errs = cl.errors(run.taps_of(0), ref, names)
    tol = TOL_FP32[fam]
    yard = cl.sub_out_yardstick(fam, tp)["fp32"]
    print(f"conformer lengths fp32 {fam} T'={tp} {cl.forms(fam, tp)['attention fp32']} tokens={len(cl.greedy(fam, tp)[0])}:",
          {k: f"{v[0]:.2e}|last {v[2]:.2e}" for k, v in errs.items()}, f"sub_out bound max({tol:.0e}, yardstick {yard:.2e})")
    note("fp32", section, fam, tp, errs)
    bad = cl.violations(errs, tol, bounds={"sub_out": (max(tol, yard), None)})
    assert not bad, (fam, tp, bad)
    assert (run.got.ids[0], run.got.frames[0]) == cl.greedy(fam, tp)


def check_bf16(models, section, fam, tp, recipe="bf16-fused-glu"):
    cfg, sd = CFGS[fam], cl.weights(fam)
    ref = cl.oracle(fam, tp, recipe)
    run = tapped_and_untapped(models(fam, "bf16"), fam, tp)
    assert run.got.enc_lens == [ref["enc_len"]] == [tp]
    assert int(run.buf.n_frames[0]) == ref["n_frames"]
    errs = cl.errors(run.taps_of(0), ref)
    yard = cl.sub_out_yardstick(fam, tp)
    form = cl.forms(fam, tp)
    print(f"conformer lengths bf16 {fam} T'={tp} {recipe} {form['attention bf16']}; {form['conv fused' if recipe != 'bf16' else 'conv unfused']}:",
          {k: f"{v[0]:.2e}|mean {v[1]:.2e}|last {v[2]:.2e}" for k, v in errs.items()},
          f"sub_out bound max({cl.TOL_BF16_MAX:.0e}, {yard['bf16_max']:.2e}) / mean max({cl.TOL_BF16_MEAN:.0e}, {yard['bf16_mean']:.2e})")
    note("bf16", section, fam, tp, errs)
    bad = cl.violations(errs, cl.TOL_BF16_MAX, cl.TOL_BF16_MEAN,
                        bounds={"sub_out": (max(cl.TOL_BF16_MAX, yard["bf16_max"]), max(cl.TOL_BF16_MEAN, yard["bf16_mean"]))})
    if cfg.espnet:
        e = cl.errors(run.taps_of(0), ref, ("ctc",))
        print(f"    ctc {e['ctc'][0]:.2e}")
        note("bf16", section, fam, tp, e)
        bad += cl.violations(e, cl.TOL_CTC_BF16)
    assert not bad, (fam, tp, bad)
    same = og.rnnt_greedy(cfg, sd, run.buf.joint_enc.cpu().numpy(), np.asarray(run.got.enc_lens, np.int32))
    assert run.got.ids == [r[0] for r in same] and run.got.frames == [r[1] for r in same]
    if cfg.espnet:
        assert len(set(run.got.frames[0])) == len(run.got.frames[0]), "ESPnet greedy emits at most one symbol per frame"


# ---- 1. the ladder ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,tp", LADDER_CASES)
def test_ladder_fp32_mode_vs_fp32_oracle(models, fam, tp):
    check_fp32(models, "ladder", fam, tp)


@pytest.mark.parametrize("fam,tp", LADDER_CASES)
def test_ladder_bf16_mode_vs_bf16_recipe_oracle(models, fam, tp):
    check_bf16(models, "ladder", fam, tp)


# ---- 2. the other conv layout --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,tp", UNFUSED_CASES)
def test_unfused_glu_bf16_mode_vs_bf16_recipe(models, fam, tp):
    model = models(fam, "bf16")
    model.ctx.set_option("fuse_glu", 0)
    try:
        check_bf16(models, "unfused_glu", fam, tp, recipe="bf16")
    finally:
        model.ctx.set_option("fuse_glu", 1)


# ---- 3. one utterance through every buffer length --------------------------------------------------------------------------------------------
ALONE = {}


def alone(models, fam, precision, tp):
    """(enc_len, enc, joint, ids, frames) of wave(fam, tp) alone in a buffer sized to it, once per (family, mode, length)"""
    key = (fam, precision, tp)
    if key not in ALONE:
        run = Run(models(fam, precision), [cl.wave(fam, tp)])
        assert run.tp_max == tp
        ALONE[key] = run.outputs(0)
        assert ALONE[key][0] == tp
    return ALONE[key]


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("fam,tp", [(fam, t) for fam in ("nemo", "espnet") for t in cl.FORM_TP])
def test_one_utterance_through_every_buffer_length_bits(models, fam, precision, tp):
    """row 0 of a buffer of 33 / 161 / 193 / 385 frames beside a full-length row == the utterance alone, bit for bit"""
    ref = alone(models, fam, precision, tp)
    ran = []
    for buf_tp in cl.FORM_BUF:
        if buf_tp < tp:
            continue
        run = Run(models(fam, precision), [cl.wave(fam, tp), cl.wave(fam, buf_tp)])
        assert run.tp_max == buf_tp and run.got.enc_lens == [tp, buf_tp]
        assert same_bits(run.outputs(0), ref), (fam, precision, tp, buf_tp)
        assert same_bits(run.outputs(1), alone(models, fam, precision, buf_tp)), (fam, precision, buf_tp, "the full-length row")
        ran.append(buf_tp)
    assert ran
    key = "attention " + precision
    print(f"conformer forms {fam} {precision} T'={tp}: alone [{cl.forms(fam, tp)[key]}] == in buffers {[(t, cl.forms(fam, t)[key]) for t in ran]}")


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("fam", ["nemo", "espnet"])
def test_ragged_batch_of_five_bits(models, fam, precision):
    run = Run(models(fam, precision), [cl.wave(fam, t) for t in cl.FORM_TP])
    assert run.tp_max == max(cl.FORM_TP) and run.got.enc_lens == list(cl.FORM_TP)
    for b, tp in enumerate(cl.FORM_TP):
        assert same_bits(run.outputs(b), alone(models, fam, precision, tp)), (fam, precision, tp)
    assert sum(len(x) for x in run.got.ids) > 10


# ---- 4. limited-context attention ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,tp", WINDOW_CASES)
def test_window_fp32_mode_vs_fp32_oracle(models, fam, tp):
    check_fp32(models, "window", fam, tp)


@pytest.mark.parametrize("fam,tp", WINDOW_CASES)
def test_window_bf16_mode_vs_bf16_recipe_oracle(models, fam, tp):
    check_bf16(models, "window", fam, tp)


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_window_257_alone_equals_inside_the_513_buffer_bits(models, precision):
    ref = alone(models, "nemo_w", precision, 257)
    run = Run(models("nemo_w", precision), [cl.wave("nemo_w", 257), cl.wave("nemo_w", 513)])
    assert run.tp_max == 513 and run.got.enc_lens == [257, 513]
    assert same_bits(run.outputs(0), ref), precision
    assert len(ref[3]) > 0


# ---- 5. position-table capacity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("fam", ["nemo", "espnet"])
def test_position_table_capacity_and_growth_bits(models, fam, precision):
    """pos_cap = 32 (the slices pos_table + (tcap - T') d and the pos_proj rows at the same offset) and the tables regrown by
    AsrModel.ensure_pos_cap == the default capacity, bit for bit, before and after the growth"""
    small, full = models(fam, precision, pos_cap=32), models(fam, precision)
    assert small.pos_cap == 32 and full.pos_cap >= 1024
    cap0 = full.pos_cap
    outs = []
    for step, tp in enumerate((20, 200, 20)):
        a = Run(small, [cl.wave(fam, tp)])
        assert small.pos_cap == (32 if step == 0 else 256), (step, small.pos_cap)
        b = Run(full, [cl.wave(fam, tp)])
        assert a.tp_max == b.tp_max == tp and a.got.enc_lens == [tp]
        assert same_bits(a.outputs(0), b.outputs(0)), (fam, precision, step, tp)
        outs.append(a.outputs(0))
    assert same_bits(outs[0], outs[2]), (fam, precision, "T' = 20 before and after the growth")
    assert full.pos_cap == cap0 and float(outs[1][1].abs().max()) > 0.1


# ---- 6. a row with no output frame ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("fam", ["nemo", "espnet"])
def test_row_without_an_output_frame_inside_a_ragged_batch(models, fam, precision):
    cfg, model = CFGS[fam], models(fam, precision)
    tps = (33, 0, 129, 9)
    waves = [cl.wave(fam, t) for t in tps]
    assert cfg.enc_frames(cfg.mel_frames(len(waves[1]))) == 0 and len(waves[1]) >= 128
    run = Run(model, waves)
    assert run.tp_max == 129 and run.got.enc_lens == list(tps)
    assert run.got.ids[1] == [] and run.got.frames[1] == []
    keep = [0, 2, 3]
    without = Run(model, [waves[b] for b in keep])
    for k, b in enumerate(keep):
        assert same_bits(run.outputs(b), without.outputs(k)), (fam, precision, b)
        assert same_bits(run.outputs(b), alone(models, fam, precision, tps[b])), (fam, precision, b)
    assert sum(len(run.got.ids[b]) for b in keep) > 0


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_buffer_without_an_output_frame_is_refused(models, precision):
    """ESPnet, 6 feature frames: T' = 0 for the whole buffer -> RS_EINVAL (the return code only)"""
    model = models("espnet", precision)
    cfg = model.cfg
    buf = model.stage([cl.wave("espnet", 0)])
    assert buf.t_max == 6 and cfg.enc_frames(buf.t_max) == 0
    with pytest.raises(capi.RsError) as e:
        model.run_device(buf)
    torch.cuda.synchronize()
    assert e.value.code == capi.RS_EINVAL
    again = Run(model, [cl.wave("espnet", 9)])                     # the context goes on working
    assert same_bits(again.outputs(0), alone(models, "espnet", precision, 9))


# ---- 7. the public path --------------------------------------------------------------------------------------------------------------------
def public_audio(cfg, tp, pad, seed):
    n = cl.samples_for(cfg, tp) - pad
    assert n > 0 and cfg.enc_frames(cfg.mel_frames(n + pad)) == tp
    return synthetic_batch(1, n / cfg.sample_rate, seed=seed)[0][0][:n]


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_nemo_transcribe_batch_equals_transcribe_across_rungs(gpu_device, precision):
    from reazonspeech_amd.nemo.asr import transcribe, transcribe_batch, audio_from_numpy, TranscribeConfig
    cfg = CFGS["nemo"]
    model = AsrModel(cfg, cl.weights("nemo"), SyntheticTokenizer(cfg.vocab_size), device="cuda:0", precision=precision)
    assert model.pad_left == model.pad_right == 8000
    audios = [audio_from_numpy(public_audio(cfg, tp, 16000, 7100 + tp), 16000) for tp in cl.PUBLIC_TP["nemo"]]
    assert len({cl.forms("nemo", tp)["attention bf16"] for tp in cl.PUBLIC_TP["nemo"]}) == 3
    together = transcribe_batch(model, audios, TranscribeConfig(verbose=False))
    for a, res in zip(audios, together):
        one = transcribe(model, a, TranscribeConfig(verbose=False))
        assert res.text == one.text
        assert [(s.token_id, s.token, s.seconds) for s in res.subwords] == [(s.token_id, s.token, s.seconds) for s in one.subwords]
        assert [(s.start_seconds, s.end_seconds, s.text) for s in res.segments] == [(s.start_seconds, s.end_seconds, s.text) for s in one.segments]
    assert sum(len(r.subwords) for r in together) > 10


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_espnet_transcribe_batch_equals_transcribe_across_rungs(gpu_device, precision):
    from reazonspeech_amd.espnet.asr import interface
    from reazonspeech_amd.espnet.asr.model import EspnetModel, synthetic_token_list, PADDING
    etr = importlib.import_module("reazonspeech_amd.espnet.asr.transcribe")
    cfg = CFGS["espnet"]
    model = EspnetModel(cfg, cl.weights("espnet"), synthetic_token_list(cfg.vocab_size, cl.WEIGHT_SEED["espnet"]), device="cuda:0", precision=precision)
    audios = [interface.AudioData(public_audio(cfg, tp, sum(PADDING), 7200 + tp), 16000) for tp in cl.PUBLIC_TP["espnet"]]
    assert len({cl.forms("espnet", tp)["attention bf16"] for tp in cl.PUBLIC_TP["espnet"]}) == 3
    together = etr.transcribe_batch(model, audios)
    for a, res in zip(audios, together):
        one = etr.transcribe(model, a, interface.TranscribeConfig(verbose=False))
        assert res.text == one.text
        assert [(s.start_seconds, s.end_seconds, s.text) for s in res.segments] == [(s.start_seconds, s.end_seconds, s.text) for s in one.segments]
        assert res.text == model.recognize(a.waveform)
    assert sum(len(r.text) for r in together) > 10
