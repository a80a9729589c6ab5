"""float64 reference of the Conformer's relative-position attention (csrc/k_attention.hip, the three float32 kernels of
csrc/k_f32.hip), plain torch on the CPU with explicit index arithmetic, the tolerance the bf16 forms are held to, the poisoned test
case both test files build and the list of bf16 cases.  tests/test_attention_ref_host.py shows that the reference agrees with
oracle/model.py's attention_core and with a literal triple loop, that a CPU emulation of the device recipe stays inside the tolerance
on every case of the GPU file and that deliberately wrong variants do not; tests/test_gpu_attention_edges.py compares the device.

Conventions: q, k, v [B][T][H][dh], pos [2T-1][H][dh] (row n is the relative position T - 1 - n, so the score of query i and key j
reads row j - i + T - 1), bias_u, bias_v [H][dh], lens [B].  att_left / att_right < 0: unbounded on that side; both < 0: full
attention, n_global is ignored.
"""
import torch

U_BF16 = 2.0 ** -8                         # unit roundoff of bf16 (8 significant bits, round to nearest)


def rb(t):
    return t.to(torch.bfloat16).to(torch.float32)


def clamp_lens(lens, T):
    return [min(max(int(n), 0), T) for n in lens]


def visible(T, lens, att_left, att_right, n_global):
    """bool [B][T][T]: query i sees key j.  Both below the (clamped) length; inside the window or one of them a global token."""
    i = torch.arange(T)[:, None]
    j = torch.arange(T)[None, :]
    win = torch.ones((T, T), dtype=torch.bool)
    if att_left >= 0 or att_right >= 0:
        if att_left >= 0:
            win = win & (i - j <= att_left)
        if att_right >= 0:
            win = win & (j - i <= att_right)
        if n_global > 0:
            win = win | (i < n_global) | (j < n_global)
    n = torch.tensor(clamp_lens(lens, T))[:, None, None]
    return win[None] & (i[None] < n) & (j[None] < n)


def q_plus_bias(q, bias, round_q):
    """q + bias as the device forms it: a float32 add, rounded to bf16 for the bf16 forms; exact (float64) for the float32 forms"""
    if round_q == "bf16":
        return rb(q.float() + bias.float()).double()
    assert round_q == "f32"
    return q.double() + bias.double()


def scores(qu, qv, k, pos, dtype=torch.float64):
    """[B][H][T][T] unmasked (qu_i . k_j + qv_i . pos[j - i + T - 1]) / sqrt(dh) in `dtype`; query i reads the table rows
    T - 1 - i .. 2T - 2 - i, one per key"""
    B, T, H, dh = k.shape
    qu, qv, k, pos = (t.to(dtype) for t in (qu, qv, k, pos))
    ac = torch.einsum("bihe,bjhe->bhij", qu, k)
    bd = torch.empty_like(ac)
    for i in range(T):
        bd[:, :, i, :] = torch.einsum("bhe,jhe->bhj", qv[:, i], pos[T - 1 - i:2 * T - 1 - i])
    return (ac + bd) * torch.tensor(dh ** -0.5, dtype=dtype)


def relpos_attention(q, k, v, pos, bias_u, bias_v, lens, att_left=-1, att_right=-1, n_global=0, round_q="bf16"):
    """(ctx, A), both float64 [B][T][H*dh]: ctx_i = sum_j p_ij v_j with p = softmax over the visible keys, A_i = sum_j p_ij |v_j|
    (what the tolerance scales with).  Lengths above T clamp to T; queries at or past their length give zeros in both.  Nothing is
    rounded but q + u and q + v under round_q = "bf16"."""
    B, T, H, dh = q.shape
    s = scores(q_plus_bias(q, bias_u, round_q), q_plus_bias(q, bias_v, round_q), k, pos)
    ok = visible(T, lens, att_left, att_right, n_global)[:, None]                # [B][1][T][T]
    s = s.masked_fill(~ok, float("-inf"))
    m = s.max(dim=-1, keepdim=True).values
    e = torch.exp(s - torch.where(torch.isinf(m), torch.zeros_like(m), m)).masked_fill(~ok, 0.0)
    den = e.sum(dim=-1, keepdim=True)
    p = e / torch.where(den > 0, den, torch.ones_like(den))
    vd = v.double()
    ctx = torch.einsum("bhij,bjhe->bihe", p, vd).reshape(B, T, H * dh)
    A = torch.einsum("bhij,bjhe->bihe", p, vd.abs()).reshape(B, T, H * dh)
    return ctx, A


def score_delta(q, k, v, pos, bias_u, bias_v, lens, att_left=-1, att_right=-1, n_global=0):
    """delta of tol_bf16: max |s_f32 - s_f64| over the visible scores + 2^-16.  The float32 scores are torch's own float32 products
    of the same bf16-rounded operands (another summation order than any kernel's); 2^-16 is the allowance for __expf."""
    B, T, H, dh = q.shape
    qu, qv = q_plus_bias(q, bias_u, "bf16"), q_plus_bias(q, bias_v, "bf16")
    ok = visible(T, lens, att_left, att_right, n_global)[:, None]
    diff = (scores(qu, qv, k, pos, torch.float32).double() - scores(qu, qv, k, pos)).abs()
    diff = diff.masked_fill(~ok, 0.0)
    return float(diff.max()) + 2.0 ** -16


def tol_bf16(ref, A, delta):
    """per element, for a bf16 context computed from bf16 probabilities and float32 scores: u (A + |ref|) + 4 delta A.
    u = 2^-8 once for the probabilities (each p_ij moves by at most u p_ij: the sum by u A) and once for the stored context
    (u |ref|); a score error of delta moves every probability by at most (e^(2 delta) - 1) p < 4 delta p (numerator and normaliser).
    Nothing here is measured on a kernel.  Zero where A is: compare valid rows only."""
    return U_BF16 * (A + ref.abs()) + 4.0 * delta * A


TOL_F32 = 2e-5                             # the float32 forms: absolute, as tests/test_gpu_fp32_mode.py::test_attention_f32


def worst_ratio(got, ref, tol):
    """max |got - ref| / tol over all elements (tol > 0 everywhere); inf when an element is NaN, so that `<= 1` never passes one"""
    r = (got.double() - ref).abs() / tol
    return float("inf") if bool(torch.isnan(r).any()) else float(r.max())


def valid_rows(x, lens):
    """the rows below each utterance's (clamped) length of x [B][T][d], concatenated"""
    T = x.shape[1]
    return torch.cat([x[b, :n] for b, n in enumerate(clamp_lens(lens, T))], dim=0)


class Case:
    """one attention problem: random q, k, v, pos (bf16-representable unless bf16_inputs=False), biases 0.3 randn, and POISONED
    padding: the frames at or past each length hold 8 randn in Q and K and the constant 100 in V.  All finite, so a key that is
    masked (weight exactly 0) still contributes exactly 0, and a key that leaks moves the output by tens.  poison=False zeroes the
    same frames instead: the reference must not change."""

    def __init__(self, T, H, dh, lens, seed, poison=True, bf16_inputs=True, pos=None):
        g = torch.Generator().manual_seed(seed)
        self.T, self.H, self.dh, self.lens, self.B = T, H, dh, list(lens), len(lens)
        B = self.B
        conv = rb if bf16_inputs else (lambda t: t)
        q, k, v = (conv(torch.randn((B, T, H, dh), generator=g)) for _ in range(3))
        drawn = conv(torch.randn((2 * T - 1, H, dh), generator=g))
        self.pos = drawn if pos is None else pos
        self.bias_u, self.bias_v = 0.3 * torch.randn((H, dh), generator=g), 0.3 * torch.randn((H, dh), generator=g)
        pq, pk = (conv(8 * torch.randn((B, T, H, dh), generator=g)) for _ in range(2))
        pad = (torch.arange(T)[None, :] >= torch.tensor(clamp_lens(lens, T))[:, None])[:, :, None, None]
        zero = torch.zeros(())
        self.q = torch.where(pad, pq if poison else zero, q)
        self.k = torch.where(pad, pk if poison else zero, k)
        self.v = torch.where(pad, torch.tensor(100.0 if poison else 0.0), v)

    def alone(self, b, n):
        """utterance b's first n frames as a batch of their own at T = n: the same rows, and the centred 2n - 1 rows of the position
        table (relative positions n - 1 .. -(n - 1)), so every visible score has the same operands as inside this batch"""
        c = object.__new__(Case)
        c.T, c.H, c.dh, c.lens, c.B = n, self.H, self.dh, [n], 1
        c.q, c.k, c.v = (t[b:b + 1, :n].contiguous() for t in (self.q, self.k, self.v))
        c.pos = self.pos[self.T - n:self.T + n - 1].contiguous()
        c.bias_u, c.bias_v = self.bias_u, self.bias_v
        return c

    def args(self):
        return self.q, self.k, self.v, self.pos, self.bias_u, self.bias_v, self.lens

    def qkv(self):
        """[B][T][3 d]: the layout of the operators' input"""
        B, T, d = self.B, self.T, self.H * self.dh
        return torch.cat([t.reshape(B, T, d) for t in (self.q, self.k, self.v)], dim=-1)


def edge_lens(T, tile):
    """T, 0, 1 and the two neighbours of the last multiple of `tile` below T, without repeats, none above T"""
    seam = tile * ((T - 1) // tile)
    out = []
    for n in (T, 0, 1, seam - 1, seam + 1):
        if 0 <= n <= T and n not in out:
            out.append(n)
    return out


def three_lens(T, tile, overlong=False):
    """the lengths of edge_lens in two batches of three utterances (the persistent and streaming cases fix B = 3):
    [T, 0, 1] and [T (T + 5 when overlong), seam - 1, seam + 1], filled up with T where T has no such length"""
    e = edge_lens(T, tile)
    return [(e[:3] + [T])[:3], ([T + 5 if overlong else T] + e[3:] + [T, T])[:3]]


# ---- the bf16 cases of tests/test_gpu_attention_edges.py: (head_dim, T, (att_left, att_right, n_global), lens) ---------------------
D_MODEL = 256                              # TINY: 2 heads of 128, or 4 of 64
FULL = (-1, -1, 0)
STAGED_T = {128: (1, 32, 33, 160, 161, 193, 321), 64: (1, 32, 33, 128, 129, 257)}
STAGED_OVERLONG = {128: 161, 64: 129}      # the T of each form whose batch also holds a length of T + 5
GEOMETRY_T = (97, 193, 257)                # head_dim 64 under every $RS_ATTN64 geometry
WINDOWS_161 = ((0, 0, 0), (5, 3, 0), (31, 0, 0), (32, 0, 0), (33, 0, 0), (0, 31, 0), (0, 32, 0), (0, 33, 0), (-1, 4, 0), (4, -1, 0),
               (20, 10, 1), (20, 10, 32), (20, 10, 33), (128, 128, 1))
WINDOWS_353 = ((20, 10, 0), (20, 10, 2), (200, 17, 0))
WINDOW_OVERLONG = (161, (5, 3, 0))
PERSIST_T = 193
STREAM_T = (1, 16, 17, 80, 81, 97, 161)
STREAM_OVERLONG = 81


def staged_cases(dh):
    return [(dh, T, FULL, edge_lens(T, 32) + ([T + 5] if T == STAGED_OVERLONG[dh] else [])) for T in STAGED_T[dh]]


def geometry_cases():
    return [(64, T, FULL, edge_lens(T, 32)) for T in GEOMETRY_T]


def window_cases(dh):
    return [(dh, T, w, edge_lens(T, 32) + ([T + 5] if (T, w) == WINDOW_OVERLONG else []))
            for T, ws in ((161, WINDOWS_161), (353, WINDOWS_353)) for w in ws]


def persist_cases(dh):
    return [(dh, PERSIST_T, FULL, lens) for lens in three_lens(PERSIST_T, 32, overlong=True)]


def stream_cases(dh):
    return [(dh, T, FULL, lens) for T in STREAM_T for lens in three_lens(T, 16, overlong=T == STREAM_OVERLONG)]


def all_bf16_cases():
    out = []
    for dh in (128, 64):
        for c in staged_cases(dh) + (geometry_cases() if dh == 64 else []) + window_cases(dh) + persist_cases(dh) + stream_cases(dh):
            if c not in out:
                out.append(c)
    return out


def make(dh, T, window, lens, poison=True, bf16_inputs=True):
    """the Case of one entry of the lists above; the seed depends on everything but the poison"""
    seed = 1000003 * (dh // 64) + 1009 * T + 31 * sum(lens) + 7 * window[0] + 3 * window[1] + window[2]
    return Case(T, D_MODEL // dh, dh, lens, seed, poison=poison, bf16_inputs=bf16_inputs)
