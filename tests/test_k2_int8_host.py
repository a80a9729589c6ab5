"""CPU: the int8 ("int8" / "int8-fp32") ONNX files of `reazonspeech.k2.asr` — onnx_lite's int8 / uint8 initializers, the quantized
reader (runtime/k2_onnx.py: read_k2_onnx_quantized) and its refusals, ORT's QInt8 weight recipe (quantize_k2_linears), and the spec
corners of the CPU restatement (tests/k2_int8_ref.py) the GPU tests check against."""
import numpy as np
import pytest
import torch

import k2_int8_ref as qr
from k2_onnx_int8_writer import write_k2_onnx_int8, quantize_matmuls
from reazonspeech_amd.runtime import k2_onnx, k2_weights as kw, onnx_lite
from reazonspeech_amd.runtime.k2_config import ZIPFORMER_TINY


def test_int8_and_uint8_initializers_round_trip(tmp_path):
    m = onnx_lite.Model()
    m.initializers["w_q"] = np.arange(-128, 128, dtype=np.int8).reshape(16, 16)
    m.initializers["z"] = np.asarray(200, np.uint8)
    m.initializers["s"] = np.asarray(0.25, np.float32)
    onnx_lite.dump(str(tmp_path / "m.onnx"), m)
    r = onnx_lite.load(str(tmp_path / "m.onnx"))
    assert r.initializers["w_q"].dtype == np.int8 and np.array_equal(r.initializers["w_q"], m.initializers["w_q"])
    assert r.initializers["z"].dtype == np.uint8 and r.initializers["z"].reshape(-1).tolist() == [200]


def test_qint8_weight_recipe():
    w = torch.tensor([[0.5, -1.27, 0.0], [1.0, 0.635, -0.005]], dtype=torch.float32)
    wq, sw, zw = kw.quantize_weight_qint8(w)
    assert zw == 0 and sw == float(np.float32(np.float32(1.27) / np.float32(127)))
    assert wq.dtype == torch.int8 and int(wq.abs().max()) == 127
    assert torch.equal(wq, torch.from_numpy(np.clip(np.rint(w.numpy() / np.float32(sw)), -127, 127).astype(np.int8)))
    zq, zs, _ = kw.quantize_weight_qint8(torch.zeros(3, 4))
    assert zs == 1.0 and int(zq.abs().max()) == 0
    cfg = ZIPFORMER_TINY
    names = kw.quantized_linears_k2(cfg)
    per_layer = 18                       # attention-weights in_proj, linear_pos, 8 modules x (in_proj, out_proj)
    assert len(names) == 2 + per_layer * sum(cfg.num_layers)
    assert not any("decoder_proj" in n or "output_linear" in n for n in names)


def files(tmp_path, cfg, sd, q, precision):
    d = {"int8": ("encoder.int8.onnx", "decoder.int8.onnx", "joiner.int8.onnx"),
         "int8-fp32": ("encoder.int8.onnx", "decoder.onnx", "joiner.int8.onnx")}[precision]
    paths = [str(tmp_path / n) for n in d]
    write_k2_onnx_int8(cfg, sd, q, *paths)
    return paths


@pytest.mark.parametrize("precision", ["int8", "int8-fp32"])
def test_quantized_reader_recovers_config_dequantized_weights_and_q(tmp_path, precision):
    cfg = ZIPFORMER_TINY
    sd = kw.synthetic_state_dict_k2(cfg, 5)
    q = kw.quantize_k2_linears(cfg, sd)
    paths = files(tmp_path, cfg, sd, q, precision)
    cfg2, sd2, q2 = k2_onnx.read_k2_onnx_quantized(*paths)
    assert cfg2 == cfg.with_(unk_id=cfg2.unk_id) and set(sd2) == set(sd) and set(q2) == set(q)
    deq = kw.dequantize_k2_linears(sd, q)
    for k in q:
        wq, sw, zw = q[k]
        wq2, sw2, zw2 = q2[k]
        assert torch.equal(wq2, wq) and sw2 == sw and zw2 == zw, k
        assert torch.equal(sd2[k + ".weight"], deq[k + ".weight"]), k
    for k in sd:
        if k.endswith("downsample.bias") or k.endswith("downsample_output.bias"):
            assert torch.allclose(torch.softmax(sd[k], 0), torch.softmax(sd2[k], 0), atol=1e-6)
        elif k[:-len(".weight")] not in q:
            assert torch.allclose(sd[k].float(), sd2[k].float(), atol=1e-6), k
    # the device tensors of the int8 mode: layout of the ".f32" copies, K padded to 32 with zeros, column sums over the real K
    w = kw.prepare_weights_k2(cfg2, sd2, 16, f32=True, i8=q2)
    for name, dev in kw.quantized_linears_k2(cfg).items():
        t = w[dev + ".i8"]
        assert t.dtype == torch.int8 and t.shape[1] % 32 == 0
        assert torch.equal(w[dev + ".i8.cs"], t.to(torch.int64).sum(1).to(torch.int32))
        assert w[dev + ".i8.q"][0] == np.float32(q2[name][1])
        if dev + ".f32" in w:
            assert w[dev + ".f32"].shape == t.shape and torch.equal(w[dev + ".f32"] == 0, (t == 0) | (w[dev + ".f32"] == 0))
    sa = w["S0.L0.sa1.out.w.i8"]
    assert sa.shape[1] == 32 and torch.all(sa[:, 24:] == 0)                   # H * 12 = 24 columns padded to 32
    assert w["pos.enc"].shape == (31, cfg.pos_dim)
    # the float reader still refuses these files, as before
    with pytest.raises(ValueError, match="quantized"):
        k2_onnx.read_k2_onnx(*paths)


def _rewrite(path, fn):
    m = onnx_lite.load(path)
    fn(m)
    onnx_lite.dump(path, m)


def test_quantized_reader_refusals(tmp_path):
    cfg = ZIPFORMER_TINY
    sd = kw.synthetic_state_dict_k2(cfg, 5)
    q = kw.quantize_k2_linears(cfg, sd)
    paths = files(tmp_path, cfg, sd, q, "int8")

    def first(m, op):
        return [n for n in m.nodes if n.op_type == op][0]

    def non_const_b(m):
        first(m, "MatMulInteger").inputs[1] = "some_activation"

    def per_channel_scale(m):
        n = first(m, "MatMulInteger")
        sw = [i for i in m.nodes if i.name == n.name[:-len("_quant")] + "_scales_mul"][0].inputs[1]
        m.initializers[sw] = np.full((m.initializers[n.inputs[1]].shape[1],), 0.01, np.float32)

    def per_channel_zero_point(m):
        n = first(m, "MatMulInteger")
        m.initializers[n.inputs[3]] = np.zeros((m.initializers[n.inputs[1]].shape[1],), np.int8)

    def no_scale_mul(m):
        n = first(m, "MatMulInteger")
        m.nodes = [i for i in m.nodes if i.name != n.name[:-len("_quant")] + "_output_scale_mul"]

    def other_op(op):
        return lambda m: m.nodes.append(onnx_lite.Node("/encoder/x/" + op, op, ["a", "b"], ["c"]))

    cases = [non_const_b, per_channel_scale, per_channel_zero_point, no_scale_mul] + [other_op(o) for o in ("QLinearMatMul", "ConvInteger", "DequantizeLinear")]
    for fn in cases:
        write_k2_onnx_int8(cfg, sd, q, *paths)
        _rewrite(paths[0], fn)
        with pytest.raises(ValueError, match="quantized"):
            k2_onnx.read_k2_onnx_quantized(*paths)
    # a quantized output_linear / decoder_proj: refused on purpose (a real export leaves them float32 Gemm nodes)
    qj = {"joiner.output_linear": kw.quantize_weight_qint8(sd["joiner.output_linear.weight"]),
          "joiner.decoder_proj": kw.quantize_weight_qint8(sd["joiner.decoder_proj.weight"])}
    for path in (paths[2], paths[1]):
        write_k2_onnx_int8(cfg, sd, q, *paths)
        _rewrite(path, lambda m: quantize_matmuls(m, qj))
        with pytest.raises(ValueError, match="quantized.*Gemm"):
            k2_onnx.read_k2_onnx_quantized(*paths)
    # float files: nothing quantized
    from k2_onnx_writer import write_k2_onnx
    write_k2_onnx(cfg, sd, *paths)
    with pytest.raises(ValueError, match="no quantized"):
        k2_onnx.read_k2_onnx_quantized(*paths)


def test_restatement_spec_corners():
    # exact .5 ties round half to even: range [0, 255] -> sx = 1, zx = 0
    x = np.asarray([[0.0, 255.0, 2.5, 3.5, 0.5, 1.5, 254.5]], np.float32)
    sx, zx = qr.range_params(x)
    assert (sx, zx) == (1.0, 0.0)
    assert qr.quantize(x, sx, zx).tolist() == [[0, 255, 2, 4, 0, 2, 254]]
    # a negative minimum sets the zero point: round(-min / sx), ties to even
    sx, zx = qr.range_params(np.asarray([-0.5, 254.5], np.float32))
    assert sx == np.float32(255.0) / np.float32(255.0) and zx == 0.0            # 0.5 -> 0 (even)
    sx, zx = qr.range_params(np.asarray([-1.5, 253.5], np.float32))
    assert zx == 2.0
    # saturation (values outside the statistics' range: rows past the length)
    assert qr.quantize(np.asarray([-1e30, 1e30, np.inf, -np.inf], np.float32), np.float32(0.01), np.float32(7)).tolist() == [0, 255, 255, 0]
    # an all-zero tensor: sx = 1, zx = 0, output = bias, no NaN
    wq = np.asarray([[1, -2, 3], [127, -127, 0]], np.int8)
    bias = np.asarray([0.25, -3.0], np.float32)
    y = qr.qlinear(np.zeros((4, 3), np.float32), wq, 0.5, 0, bias)
    assert np.array_equal(y, np.broadcast_to(bias, (4, 2)))
    # padding rows are excluded from the statistics, and quantized with the utterance's own scale
    x = np.asarray([[1.0, -2.0, 0.5], [0.25, 0.0, -1.0], [1e6, -1e6, 3e7]], np.float32)
    y = qr.qlinear(x, wq, 0.5, 3, bias, rows=2)
    assert np.array_equal(y[:2], qr.qlinear(x[:2], wq, 0.5, 3, bias))
    sx, zx = qr.range_params(x[:2])
    assert qr.quantize(x[2:], sx, zx).tolist() == [[255, 0, 255]]
    # the integer path equals the float64 definition (x_q - zx)(W - zw) exactly here (small integers)
    xq = qr.quantize(x[:2], sx, zx).astype(np.float64) - zx
    want = ((xq @ (wq.astype(np.float64) - 3).T).astype(np.float32) * np.float32(np.float32(sx) * np.float32(0.5)) + bias).astype(np.float32)
    assert np.array_equal(y[:2], want)
