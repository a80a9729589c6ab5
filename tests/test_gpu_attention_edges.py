"""-m gpu: every form of the Conformer's relative-position attention (csrc/k_attention.hip and the three float32 kernels of
csrc/k_f32.hip), one operator call at a time through the C ABI, against the float64 reference of tests/attention_ref.py
(tests/test_attention_ref_host.py shows on the CPU that the reference and the tolerance are right and that they reject a padding
mask, a window edge, a global-token count or a position index off by one, u and v swapped and a dropped key block or chunk).

  kernel form                                         reached by                                                  test
  relpos_attention_kernel<128,0,0>                    head_dim 128, full attention                                test_staged_full
  relpos_attention_kernel<64,0,0,4>                   head_dim 64, default RS_ATTN64, T > 32; "4,4", "4,2"        test_staged_full, test_attn64_geometries
  relpos_attention_kernel<64,0,0,2>                   head_dim 64 at T <= 32 (one wave); "2,1", "2,2"             test_staged_full, test_attn64_geometries
  relpos_attention_kernel<64,0,0,3>                   RS_ATTN64 = "3,2", "3,4"                                    test_attn64_geometries
  relpos_attention_kernel<64,0,0>                     RS_ATTN64 = "0" (six key blocks, up to six waves)           test_attn64_geometries
  relpos_attention_kernel<128 / 64,0,1>  (WINDOW)     att_left >= 0 or att_right >= 0                             test_window
  relpos_attention_kernel<128,0,0,0,1>  (PERSIST)     RS_ATTN_PERSIST = 2, 3, 5, head_dim 128                     test_persistent
  relpos_attention_kernel<64,0,0,0 / 2 / 3 / 4,1>     the same at head_dim 64 under "0", "2,2", "3,2", "4,4"      test_persistent
  relpos_attention_stream_kernel<128 / 64,5,3,.,0>    RS_ATTN_STREAM = 1                                          test_streaming
  attention_f32_mfma_kernel<128 / 64>                 float32, full attention                                     test_f32_mfma
  attention_f32_keys_kernel<4>                        float32, T <= 256: windowed, or full + RS_ATTN_F32_KEYS     test_f32_keys
  attention_f32_keys_kernel<8>                        the same at 256 < T <= 512                                  test_f32_keys
  attention_f32_keys_kernel<0>                        float32, windowed at T > 512 (scores computed twice; the bits of <4 / 8>)   test_f32_keys_long,
                                                                                                                  test_f32_limited_context_across_the_512_seam
  attention_f32_kernel<1 / 2>                         RS_ATTN_F32_OLD at T = 65 (head_dim 64 / 128)               test_f32_first_form
  attention_f32_kernel<4>                             head_dim 256: no Context has it (TINY's d_model 256 would need one head, and the
                                                      bf16 attention the Context also sets up builds 128 and 64 only); not reached
  relpos_attention_kernel<128,1,0>  (TRACE)           the phase-timestamp debug hook of scripts/attn_trace.py; not a production form, not run here
  relpos_attention_stream_kernel<.,1>   (DBG)         RS_ATTN_STREAM = 1 + 16 x mask leaves phases out on purpose (wrong results); not run here

Rules of every case.  The output buffer has 8 rows past B * T holding a sentinel that must survive.  Every valid row is compared
and every row at or past its utterance's length must be exactly 0.  The padded frames are POISONED (8 randn in Q and K, 100 in
V), so a key that leaks past a length shows as an error of tens.  A batch holds the lengths T, 0, 1 and the two neighbours of the
last 32-row (streaming, float32 MFMA: 16-row; float32 keys / first form: 64-key) seam below T, and in one case per form a length of
T + 5, which must behave as T (the reference clamps it).  One-sided windows (att_left = -1 with att_right >= 0 and the reverse) are
accepted by Context and are run.  bf16 forms: err <= u (A + |ref|) + 4 delta A per element (attention_ref.tol_bf16); float32
forms: 2e-5 absolute.  Forms that promise the same values (the RS_ATTN64 geometries, the persistent launch, an utterance alone or
inside a longer batch) are held to value equality, which tolerates only the sign of a zero.
"""
import contextlib

import pytest
import torch

import attention_ref as ar
from knobs import knob
from reazonspeech_amd.runtime import capi
from reazonspeech_amd.runtime.config import TINY

pytestmark = pytest.mark.gpu
SENTINEL = 7.0
PAD = 8
WORST = {}                                  # kernel form -> worst observed err / tol
GEOMETRIES = ["0", "2,1", "2,2", "3,2", "3,4", "4,2", "4,4"]
W1 = (20, 10, 1)                            # the window of the float32 limited-context cases


@pytest.fixture(scope="module")
def contexts(gpu_device):
    """Context of (head_dim, window), made on first use, closed at the end; the summary of the module is printed there"""
    made = {}

    def get(dh, window=ar.FULL):
        if (dh, window) not in made:
            made[dh, window] = capi.Context(TINY.with_(n_heads=ar.D_MODEL // dh, att_left=window[0], att_right=window[1],
                                                       n_global=window[2]), 0)
        return made[dh, window]
    yield get
    for c in made.values():
        c.close()
    print("\nworst err / tol per kernel form:")
    for form in sorted(WORST):
        print(f"  {form:<52s} {WORST[form]:.3f}")


def sync():
    torch.cuda.synchronize()


def same_values(a, b):
    return bool((a.float() == b.float()).all())


@contextlib.contextmanager
def switches(lib, **settings):
    """the named switches at these values for the calls inside; RS_ATTN64 takes the variable's text "kbc[,nw]" and sets both rows"""
    with contextlib.ExitStack() as stack:
        for name, value in settings.items():
            if name == "RS_ATTN64" and value is not None:
                kbc, _, nw = value.partition(",")
                stack.enter_context(knob(lib, "RS_ATTN64", int(kbc)))
                stack.enter_context(knob(lib, "RS_ATTN64_NW", int(nw) if nw else 4))
            elif value is not None:
                stack.enter_context(knob(lib, name, value))
        yield


def run(c, case, dev, f32=False):
    """one operator call on `case` -> [B][T][d] on the CPU; the rows past B * T must keep the sentinel"""
    B, T, d = case.B, case.T, case.H * case.dh
    dt = torch.float32 if f32 else torch.bfloat16
    out = torch.full((B * T + PAD, d), SENTINEL, dtype=dt, device=dev)
    args = (case.qkv().reshape(B * T, 3 * d).to(dt).to(dev), case.pos.reshape(2 * T - 1, d).to(dt).to(dev),
            case.bias_u.reshape(-1).to(dev), case.bias_v.reshape(-1).to(dev), torch.tensor(case.lens, dtype=torch.int32).to(dev), B, T, out)
    (c.attention_f32 if f32 else c.attention)(*args)
    sync()
    assert (out[B * T:].float() == SENTINEL).all(), "rows past B * T were written"
    return out[:B * T].cpu().view(B, T, d)


_REF = {}


def reference(case, window, f32):
    """(ref, tol) of a case, computed once"""
    key = (case.dh, case.T, window, tuple(case.lens), f32, float(case.q.double().sum()))
    if key not in _REF:
        ref, A = ar.relpos_attention(*case.args(), *window, round_q="f32" if f32 else "bf16")
        tol = torch.full_like(ref, ar.TOL_F32) if f32 else ar.tol_bf16(ref, A, ar.score_delta(*case.args(), *window))
        _REF[key] = (ref, tol)
    return _REF[key]


def check(form, case, window, got, f32=False):
    ref, tol = reference(case, window, f32)
    for b, n in enumerate(ar.clamp_lens(case.lens, case.T)):
        assert (got[b, n:] == 0).all(), (form, case.T, window, case.lens, b, "a row at or past the length is not zero")
    r = ar.worst_ratio(ar.valid_rows(got, case.lens), ar.valid_rows(ref, case.lens), ar.valid_rows(tol, case.lens))
    WORST[form] = max(WORST.get(form, 0.0), r)
    print(f"{form} T={case.T} window={window} lens={case.lens}: err / tol = {r:.3f}")
    assert r <= 1.0, (form, case.T, window, case.lens, r)


# ---- bf16, the staged kernel, full attention ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dh,T,window,lens", ar.staged_cases(128) + ar.staged_cases(64))
def test_staged_full(contexts, gpu_device, dh, T, window, lens):
    """head_dim 128: one query block becomes two (32 / 33), the register-transposing stage_kv hands over to the one-item restaging
    loop (160 / 161), a second workgroup (193), three chunks (321).  head_dim 64 at the default geometry: KBC 2 with one wave up to
    T = 32, then 4 key blocks x up to 4 waves: the chunk seam is 128 / 129, the second workgroup too; 257: three chunks.
    Two cases of this list found faults in the kernel as it was (profiles/pr_attention_edges_gpu.txt): the length of T + 5 at T = 161
    leaked the clamped rows past T into the softmax (err / tol 136), and the length of 0 in the two-row batch of T = 1 at
    head_dim 64 made stage_kv load V rows from before the qkv buffer."""
    case = ar.make(dh, T, window, lens)
    check(f"staged full, head_dim {dh}", case, window, run(contexts(dh), case, gpu_device))


@pytest.mark.parametrize("dh,T,window,lens", ar.geometry_cases())
def test_attn64_geometries(contexts, gpu_device, dh, T, window, lens):
    c = contexts(64)
    case = ar.make(dh, T, window, lens)
    want = run(c, case, gpu_device)
    check("staged full, head_dim 64", case, window, want)
    for text in GEOMETRIES:
        with switches(c.lib, RS_ATTN64=text):
            got = run(c, case, gpu_device)
        check(f"staged full, head_dim 64, RS_ATTN64={text}", case, window, got)
        assert same_values(got, want), f"RS_ATTN64={text} != the default geometry at T={T}"


def test_attn64_rejects_a_geometry_that_is_not_built(contexts, gpu_device):
    c = contexts(64)
    case = ar.make(64, 64, ar.FULL, [64, 0, 1])
    with switches(c.lib, RS_ATTN64="5,4"):
        out = torch.full((3 * 64 + PAD, ar.D_MODEL), SENTINEL, dtype=torch.bfloat16, device=gpu_device)
        z = torch.zeros((3 * 64, 3 * ar.D_MODEL), dtype=torch.bfloat16, device=gpu_device)
        with pytest.raises(capi.RsError):
            c.attention(z, z, torch.zeros(ar.D_MODEL, device=gpu_device), torch.zeros(ar.D_MODEL, device=gpu_device),
                        torch.tensor([64, 0, 1], dtype=torch.int32).to(gpu_device), 3, 64, out)
        sync()
        assert (out.float() == SENTINEL).all(), "a refused geometry launched something"
    check("staged full, head_dim 64", case, ar.FULL, run(c, case, gpu_device))      # the switch is back: the default runs


# ---- bf16, WINDOW --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dh,T,window,lens", ar.window_cases(128) + ar.window_cases(64))
def test_window(contexts, gpu_device, dh, T, window, lens):
    """T = 161: a window edge on, one short of and one past a 32-key block edge on either side (w_lo / w_hi, wg_lo / wg_hi), the
    diagonal alone, one-sided windows, global tokens filling one block exactly and spilling into the next (gb_hi).  T = 353: whole
    chunks are skipped and bd_for rebuilds the lower half of the position block after them."""
    case = ar.make(dh, T, window, lens)
    check(f"staged WINDOW, head_dim {dh}", case, window, run(contexts(dh, window), case, gpu_device))


# ---- bf16, the persistent launch ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dh", [128, 64])
def test_persistent(contexts, gpu_device, dh):
    """B = 3 at T = 193: 12 (head_dim 128) or 24 / 48 / 24 items (head_dim 64 at 6 / 2 / 4 waves) on 2, 3 and 5 resident workgroups:
    with 5 the last round is short"""
    c = contexts(dh)
    for _, T, window, lens in ar.persist_cases(dh):
        case = ar.make(dh, T, window, lens)
        want = run(c, case, gpu_device)
        check(f"staged full, head_dim {dh}", case, window, want)
        for text in ([None] if dh == 128 else ["0", "2,2", "3,2", "4,4"]):
            for resident in (2, 3, 5):
                with switches(c.lib, RS_ATTN64=text, RS_ATTN_PERSIST=resident):
                    got = run(c, case, gpu_device)
                check(f"persistent, head_dim {dh}", case, window, got)
                assert same_values(got, want), f"RS_ATTN_PERSIST={resident} (RS_ATTN64={text}) != the default launch, lens={lens}"


# ---- bf16, the streaming kernel -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dh,T,window,lens", ar.stream_cases(128) + ar.stream_cases(64))
def test_streaming(contexts, gpu_device, dh, T, window, lens):
    """16-query tiles, five waves per group (80 / 81), a second group's worth of tiles (97), a three-slot ring that wraps (161: six
    key blocks); n_items = groups x heads x 3 is 6, 12 or 18 with two heads and 12, 24 or 36 with four: the grid is padded to a
    multiple of 8 in every case but the 24 of T = 81 and 97 with four heads"""
    c = contexts(dh)
    case = ar.make(dh, T, window, lens)
    with switches(c.lib, RS_ATTN_STREAM=1):
        got = run(c, case, gpu_device)
    check(f"streaming, head_dim {dh}", case, window, got)


# ---- float32 -------------------------------------------------------------------------------------------------------------------------
def f32_case(dh, T, window, tile, overlong=False):
    return ar.make(dh, T, window, ar.edge_lens(T, tile) + ([T + 5] if overlong else []), bf16_inputs=False)


@pytest.mark.parametrize("T", [1, 15, 16, 17, 63, 64, 65, 161])
@pytest.mark.parametrize("dh", [128, 64])
def test_f32_mfma(contexts, gpu_device, dh, T):
    case = f32_case(dh, T, ar.FULL, 16, overlong=T == 65)
    check(f"f32 mfma<{dh}>", case, ar.FULL, run(contexts(dh), case, gpu_device, f32=True), f32=True)


@pytest.mark.parametrize("T", [64, 65, 256, 257, 512])
@pytest.mark.parametrize("dh", [128, 64])
def test_f32_keys(contexts, gpu_device, dh, T):
    """64 keys per lane chunk: NCH = 4 up to T = 256, 8 up to 512; full attention under RS_ATTN_F32_KEYS, limited context as it runs"""
    nch = 4 if T <= 256 else 8
    case = f32_case(dh, T, ar.FULL, 64, overlong=T == 65)
    c = contexts(dh)
    with switches(c.lib, RS_ATTN_F32_KEYS=1):
        got = run(c, case, gpu_device, f32=True)
    check(f"f32 keys<{nch}> full, head_dim {dh}", case, ar.FULL, got, f32=True)
    case = f32_case(dh, T, W1, 64, overlong=T == 65)
    check(f"f32 keys<{nch}> windowed, head_dim {dh}", case, W1, run(contexts(dh, W1), case, gpu_device, f32=True), f32=True)


@pytest.mark.parametrize("dh", [128, 64])
def test_f32_first_form(contexts, gpu_device, dh):
    """one wave per query row: under RS_ATTN_F32_OLD at T = 65 (full and limited context)"""
    for window in (ar.FULL, W1):
        case = f32_case(dh, 65, window, 64, overlong=True)
        c = contexts(dh, window)
        with switches(c.lib, RS_ATTN_F32_OLD=1):
            got = run(c, case, gpu_device, f32=True)
        check(f"f32 first form<{dh // 64}>", case, window, got, f32=True)


@pytest.mark.parametrize("dh", [128, 64])
def test_f32_keys_long(contexts, gpu_device, dh):
    """limited-context attention above T = 512 — the production path of long recordings in the float32 mode:
    attention_f32_keys_kernel<0>, the keys walked 64 at a time with the scores computed twice"""
    case = f32_case(dh, 513, W1, 64)
    check(f"f32 keys<0> windowed, head_dim {dh}", case, W1, run(contexts(dh, W1), case, gpu_device, f32=True), f32=True)


# ---- the content of the padding is never read into a result -------------------------------------------------------------------------
@pytest.mark.parametrize("dh", [128, 64])
def test_poison_invariance(contexts, gpu_device, dh):
    """the valid rows with poisoned padding == the valid rows with zeroed padding, one case per form"""
    lens = ar.edge_lens(193, 32)
    runs = [("staged full", ar.FULL, {}, False), ("staged WINDOW", (20, 10, 2), {}, False), ("persistent", ar.FULL, {"RS_ATTN_PERSIST": 5}, False),
            ("streaming", ar.FULL, {"RS_ATTN_STREAM": 1}, False), ("f32 mfma", ar.FULL, {}, True), ("f32 keys", W1, {}, True),
            ("f32 first form", W1, {"RS_ATTN_F32_OLD": 1}, True)]
    for form, window, settings, f32 in runs:
        c = contexts(dh, window)
        got = []
        for poison in (True, False):
            case = ar.make(dh, 193, window, lens, poison=poison, bf16_inputs=not f32)
            with switches(c.lib, **settings):
                got.append(run(c, case, gpu_device, f32=f32))
        assert same_values(ar.valid_rows(got[0], lens), ar.valid_rows(got[1], lens)), f"{form}, head_dim {dh}: the padding's content changed valid rows"
        check(f"{form}, head_dim {dh} (zeroed padding)", case, window, got[1], f32=f32)


# ---- an utterance's rows do not depend on the batch around it -----------------------------------------------------------------------
def in_and_out(contexts, dev, dh, n, T, window, f32, settings=None):
    """rows 0 .. n-1 of utterance 1 inside a batch padded to T, and the same utterance alone at T = n"""
    big = ar.make(dh, T, window, [T, n, max(n // 3, 1)], bf16_inputs=not f32)
    c = contexts(dh, window)
    with switches(c.lib, **(settings or {})):
        inside, alone = run(c, big, dev, f32=f32), run(c, big.alone(1, n), dev, f32=f32)
    return big, inside, alone


@pytest.mark.parametrize("dh", [128, 64])
def test_batch_invariance(contexts, gpu_device, dh):
    """staged full (n = 170 alone is one workgroup of six waves and two chunks; inside T = 225 it is part of two workgroups), the
    head_dim-64 default also across its T <= 32 geometry, staged WINDOW, float32 MFMA, float32 keys on both sides of T = 256"""
    runs = [("staged full", 170, 225, ar.FULL, False, None), ("staged full", 30, 97, ar.FULL, False, None),
            ("staged WINDOW", 170, 225, (20, 10, 1), False, None), ("f32 mfma", 70, 161, ar.FULL, True, None),
            ("f32 keys windowed", 100, 256, W1, True, None), ("f32 keys windowed", 100, 257, W1, True, None),
            ("f32 keys windowed", 300, 400, W1, True, None), ("f32 keys full", 100, 256, ar.FULL, True, {"RS_ATTN_F32_KEYS": 1}),
            ("f32 keys full", 100, 257, ar.FULL, True, {"RS_ATTN_F32_KEYS": 1}), ("f32 keys full", 300, 400, ar.FULL, True, {"RS_ATTN_F32_KEYS": 1})]
    for form, n, T, window, f32, settings in runs:
        big, inside, alone = in_and_out(contexts, gpu_device, dh, n, T, window, f32, settings)
        check(f"{form}, head_dim {dh} (batch invariance)", big, window, inside, f32=f32)
        assert same_values(inside[1, :n], alone[0]), f"{form}, head_dim {dh}: n={n} alone != inside T={T}"


@pytest.mark.parametrize("dh", [128, 64])
def test_f32_limited_context_across_the_512_seam(contexts, gpu_device, dh):
    """T <= 512 takes attention_f32_keys_kernel<4 / 8> (scores in registers), T > 512 attention_f32_keys_kernel<0> (scores computed twice):
    one kernel body, the same summation orders, so an utterance's values do not change with its batch's padded length across that seam; both sides are
    held to the float32 tolerance"""
    for T in (512, 513):
        big, inside, alone = in_and_out(contexts, gpu_device, dh, 300, T, W1, True)
        check(f"f32 limited context at T={T}, head_dim {dh}", big, W1, inside, f32=True)
        small = big.alone(1, 300)
        check(f"f32 keys<8> windowed, head_dim {dh}", small, W1, alone, f32=True)
        assert same_values(inside[1, :300], alone[0]), f"f32 keys windowed, head_dim {dh}: n=300 alone != inside T={T}"
        differ = int((inside[1, :300] != alone[0]).sum())
        print(f"head_dim {dh}: n=300 alone vs inside T={T}: {differ} of {alone.numel()} elements differ, by at most "
              f"{float((inside[1, :300] - alone[0]).abs().max()):.3g}")
