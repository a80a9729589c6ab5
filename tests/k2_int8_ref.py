"""CPU restatement of onnxruntime's int8 Zipformer graph (the "int8" / "int8-fp32" files of `reazonspeech.k2.asr`), the checker of
csrc/k_int8.hip and of the int8 mode.  TEST INFRASTRUCTURE.

[UPSTREAM] ONNX DynamicQuantizeLinear, per tensor (here: per utterance, the graph sees one utterance per call):
    sx = (max(0, max x) - min(0, min x)) / 255  (onnxruntime: 1 when the range is empty), zx = saturate(round(-min(0, min x) / sx)),
    xq = saturate(round(x / sx) + zx),  round = half to even, saturate = [0, 255]
and the rest of a quantized MatMul: the integer products (exact), ONE conversion to float32, ONE float32 multiply by fl(sx sw),
the bias Add, then whatever followed the MatMul in the float graph.  The integer sums are formed in float64 (|terms| <= 255 * 255,
sums < 2^53: exact in any order).  The Zipformer forward is oracle/zipformer.py's building blocks in float32 with every quantized
Linear (runtime/k2_weights.py: quantized_linears_k2) replaced by `qlinear`; one utterance per call."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import zipformer as oz


def range_params(x):
    """(sx, zx) of DynamicQuantizeLinear over all of x (float32 arithmetic)"""
    x = np.asarray(x, np.float32)
    mn = np.float32(min(float(x.min()), 0.0)) if x.size else np.float32(0)
    mx = np.float32(max(float(x.max()), 0.0)) if x.size else np.float32(0)
    sx = np.float32(1.0) if mx == mn else np.float32(np.float32(mx - mn) / np.float32(255.0))
    zx = np.float32(np.rint(np.clip(np.float32(np.float32(0.0) - np.float32(mn / sx)), 0, 255)))
    return sx, zx


def quantize(x, sx, zx):
    """xq = saturate(round(x / sx) + zx) as uint8 (x / sx correctly rounded in float32, round half to even)"""
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        v = np.rint(x / np.float32(sx)).astype(np.float32) + np.float32(zx)
    return np.clip(np.nan_to_num(v, nan=0.0), 0, 255).astype(np.uint8)


def qlinear_rows(x, wq, sw, zw, sx, zx, bias=None):
    """the quantized MatMul with given (sx, zx): x f32 [M][K], wq int8 [N][K] -> f32 [M][N] before any activation"""
    xq = quantize(x, sx, zx).astype(np.float64) - float(zx)
    wd = np.asarray(wq, np.float64) - float(zw)
    acc = xq @ wd.T                                                  # exact integers
    assert np.all(np.abs(acc) < 2 ** 31)
    f = acc.astype(np.int64).astype(np.float32)                       # Cast: int32 -> float32, round to nearest even
    f = f * np.float32(np.float32(sx) * np.float32(sw))
    if bias is not None:
        f = f + np.asarray(bias, np.float32)
    return f


def qlinear(x, wq, sw, zw, bias=None, rows=None):
    """one utterance's quantized Linear: statistics over x[:rows] (all rows by default), applied to every row"""
    x = np.asarray(x, np.float32)
    sx, zx = range_params(x[:rows] if rows is not None else x)
    return qlinear_rows(x, wq, sw, zw, sx, zx, bias)


# ---- the int8 Zipformer (oracle/zipformer.py with the quantized Linears replaced) -----------------------------------------------
def _ql(x, q, sd, name, act=None):
    wq, sw, zw = q[name]
    b = sd.get(name + ".bias")
    y = torch.from_numpy(qlinear(x.numpy(), wq.numpy(), sw, zw, None if b is None else b.numpy()))
    return act(y) if act is not None else y


def attention_weights(cfg, sd, q, L, x, pe_fn, heads):
    T = x.shape[0]
    qd, pd = cfg.query_head_dim, cfg.pos_head_dim
    u = _ql(x, q, sd, L + "self_attn_weights.in_proj")
    qq = u[:, :heads * qd].reshape(T, heads, qd).permute(1, 0, 2)
    k = u[:, heads * qd:2 * heads * qd].reshape(T, heads, qd).permute(1, 0, 2)
    p = u[:, 2 * heads * qd:].reshape(T, heads, pd).permute(1, 0, 2)
    pos = _ql(pe_fn(T), q, sd, L + "self_attn_weights.linear_pos")             # the utterance's own 2 T - 1 rows, its own scale
    pos = pos.reshape(2 * T - 1, heads, pd).permute(1, 2, 0)
    ps = p @ pos
    i = torch.arange(T).unsqueeze(1)
    j = torch.arange(T).unsqueeze(0)
    ps = ps.gather(2, (j - i + T - 1).unsqueeze(0).expand(heads, T, T))
    return (qq @ k.transpose(1, 2) + ps).softmax(dim=-1)


def encoder_layer(cfg, sd, q, L, x, pe_fn, heads):
    x0 = x
    w = attention_weights(cfg, sd, q, L, x, pe_fn, heads)

    def ff(name, x):
        return _ql(_ql(x, q, sd, name + ".in_proj", oz.swoosh_l), q, sd, name + ".out_proj")

    def na(x):
        s, v, y = _ql(x, q, sd, L + "nonlin_attention.in_proj").chunk(3, dim=1)
        return _ql((w[0] @ (v * torch.tanh(s))) * y, q, sd, L + "nonlin_attention.out_proj")

    def sa(name, x):
        T = x.shape[0]
        v = _ql(x, q, sd, name + ".in_proj").reshape(T, heads, -1).permute(1, 0, 2)
        return _ql((w @ v).permute(1, 0, 2).reshape(T, -1), q, sd, name + ".out_proj")

    def cm(name, x):
        a, s = _ql(x, q, sd, name + ".in_proj").chunk(2, dim=1)
        g = a * torch.sigmoid(s)
        dw = sd[name + ".depthwise_conv.weight"]
        c = F.conv1d(g.t()[None], dw, sd[name + ".depthwise_conv.bias"], padding=dw.shape[-1] // 2, groups=dw.shape[0])[0].t()
        return _ql(oz.swoosh_r(c), q, sd, name + ".out_proj")

    x = x + ff(L + "feed_forward1", x)
    x = x + na(x)
    x = x + sa(L + "self_attn1", x)
    x = x + cm(L + "conv_module1", x)
    x = x + ff(L + "feed_forward2", x)
    x = oz.bypass(x0, x, sd[L + "bypass_mid.bypass_scale"])
    x = x + sa(L + "self_attn2", x)
    x = x + cm(L + "conv_module2", x)
    x = x + ff(L + "feed_forward3", x)
    x = oz.bias_norm(x, sd[L + "norm.bias"], sd[L + "norm.log_scale"])
    return oz.bypass(x0, x, sd[L + "bypass.bypass_scale"])


def encoder_embed(cfg, sd, q, feats):
    """oracle/zipformer.py encoder_embed (float32 convolutions) with its `out` Linear quantized"""
    E = "encoder_embed."
    x = feats[None, None]
    x = oz.swoosh_r(F.conv2d(x, sd[E + "conv.0.weight"], sd[E + "conv.0.bias"], padding=(0, 1)))
    x = oz.swoosh_r(F.conv2d(x, sd[E + "conv.4.weight"], sd[E + "conv.4.bias"], stride=2))
    x = oz.swoosh_r(F.conv2d(x, sd[E + "conv.7.weight"], sd[E + "conv.7.bias"], stride=(1, 2)))
    c3 = x.shape[1]
    y = F.conv2d(x, sd[E + "convnext.depthwise_conv.weight"], sd[E + "convnext.depthwise_conv.bias"], padding=3, groups=c3)
    y = oz.swoosh_l(F.conv2d(y, sd[E + "convnext.pointwise_conv1.weight"], sd[E + "convnext.pointwise_conv1.bias"]))
    y = F.conv2d(y, sd[E + "convnext.pointwise_conv2.weight"], sd[E + "convnext.pointwise_conv2.bias"])
    x = x + y
    _, c, t, f = x.shape
    out = _ql(x.transpose(1, 2).reshape(t, c * f), q, sd, E + "out")
    return oz.bias_norm(out, sd[E + "out_norm.bias"], sd[E + "out_norm.log_scale"])


def forward(cfg, sd, q, wav, taps=None):
    """wav f32[L] -> dict(feats, enc, joint_enc) of the int8 graph; sd holds the float tensors (the dequantized weights of the
    quantized Linears are not used), q = {Linear name: (Wq int8 [out][in], sw, zw)}"""
    pe_cache = {}

    def pe_fn(T):
        if T not in pe_cache:
            pe_cache[T] = torch.from_numpy(oz.compact_rel_pos_table(cfg, T).astype(np.float32))
        return pe_cache[T]

    with torch.no_grad():
        wav = torch.as_tensor(wav, dtype=torch.float32).reshape(-1)
        feats = oz.fbank(cfg, wav)
        x = encoder_embed(cfg, sd, q, feats)
        if taps is not None:
            taps["embed"] = x.clone()
        outputs = []
        for s in range(cfg.n_stacks):
            d, ds, heads = cfg.encoder_dim[s], cfg.downsampling[s], cfg.num_heads[s]
            x = oz.convert_channels(x, d)
            src = x
            if ds > 1:
                x = oz.simple_downsample(x, sd[f"encoder.encoders.{s}.downsample.bias"], ds)
            for j in range(cfg.num_layers[s]):
                x = encoder_layer(cfg, sd, q, oz.layer_prefix(cfg, s, j), x, pe_fn, heads)
            if ds > 1:
                up = x.unsqueeze(1).expand(-1, ds, -1).reshape(-1, d)[:src.shape[0]]
                x = oz.bypass(src, up, sd[f"encoder.encoders.{s}.out_combiner.bypass_scale"])
            outputs.append(x)
            if taps is not None:
                taps[f"S{s}"] = x.clone()
        pieces, cur = [outputs[-1]], cfg.encoder_dim[-1]
        for s in range(cfg.n_stacks - 2, -1, -1):
            if cfg.encoder_dim[s] > cur:
                pieces.append(outputs[s][:, cur:cfg.encoder_dim[s]])
                cur = cfg.encoder_dim[s]
        enc = oz.simple_downsample(torch.cat(pieces, dim=1), sd["encoder.downsample_output.bias"], cfg.output_downsampling)
        f = _ql(enc, q, sd, "joiner.encoder_proj")
    return {"feats": feats, "enc": enc, "joint_enc": f}


def greedy_with_margins(cfg, sd, f):
    """oracle/zipformer.py greedy_search, also returning the smallest top-1 / top-2 logit gap over its decisions -> (ids, frames,
    margins per frame)"""
    wo, bo = sd["joiner.output_linear.weight"], sd["joiner.output_linear.bias"]
    hist = [-1] * (cfg.context_size - 1) + [cfg.blank_id]
    ids, frames, margins = [], [], []
    with torch.no_grad():
        g = oz.decoder_out(cfg, sd, hist[-cfg.context_size:])
        for t in range(f.shape[0]):
            logits = torch.tanh(f[t] + g) @ wo.t() + bo
            top = torch.topk(logits, 2).values
            margins.append(float(top[0] - top[1]))
            y = int(torch.argmax(logits))
            if y != cfg.blank_id and y != cfg.unk_id:
                ids.append(y)
                frames.append(t)
                hist.append(y)
                g = oz.decoder_out(cfg, sd, hist[-cfg.context_size:])
    return ids, frames, margins
