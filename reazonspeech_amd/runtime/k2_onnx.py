"""From the three ONNX files of a `reazonspeech-k2-v2` repository (pkg/k2-asr/src/huggingface.py:41-66) to an icefall-style state
dict + ZipformerConfig, without onnx / onnxruntime / sherpa-onnx (runtime/onnx_lite.py).

[UPSTREAM, unverifiable here — no such file has ever been seen by this code] what icefall's export-onnx.py produces
(torch.onnx.export of OnnxEncoder(encoder, encoder_embed, encoder_proj), OnnxDecoder(decoder, decoder_proj),
OnnxJoiner(output_linear) after convert_scaled_to_non_scaled):
  * convolution weights / biases, Linear biases, embeddings and plain parameters used as they are (bypass_scale, BiasNorm.bias)
    keep their module names as initializer names;
  * a Linear's weight is the constant B operand of a MatMul (stored transposed, [in][out]) under an anonymous name; the NODE name
    carries the module scope ("/encoder/encoders.0/layers.0/feed_forward1/in_proj/MatMul");
  * constant-folded expressions lose their parameter: BiasNorm's exp(log_scale) is a scalar operand of a Mul in the norm's scope,
    SimpleDownsample's softmax(bias) a [ds, 1, 1] operand of a Mul in the downsample's scope (log of it is the bias up to a
    constant, which softmax ignores).
The architecture is not in the metadata of an offline Zipformer2 export: it is derived from the tensor shapes.
`read_k2_onnx` refuses quantized graphs (the "int8" / "int8-fp32" precisions); `read_k2_onnx_quantized` reads them.

[UPSTREAM, unverifiable here] the int8 files: icefall's export-onnx.py runs onnxruntime.quantization.quantize_dynamic(
op_types_to_quantize=["MatMul"], weight_type=QInt8) on the float files.  Only MatMuls whose B operand is a constant are rewritten
(MatMulConstBOnly): every Linear applied to a 3-D tensor — in the encoder file all the encoder's Linears, linear_pos and
encoder_proj.  OnnxDecoder / OnnxJoiner squeeze to 2-D, so decoder_proj and output_linear export as Gemm and stay float32;
convolutions and attention's activation x activation products stay float32.  Each rewritten MatMul becomes
    DynamicQuantizeLinear(x) -> (xq uint8, sx, zx);  MatMulInteger(xq, Wq int8 [K][N], zx, zw) -> int32;  Cast -> float;
    Mul(., Mul(sx, sw));  the original bias Add
with a per-tensor weight scale sw and zero point zw (QInt8's default is symmetric, zw = 0; nothing here relies on that)."""
import math
import re

import numpy as np
import torch

from . import onnx_lite
from .config import UnsupportedCheckpoint
from .k2_config import ZipformerConfig
from .k2_weights import expected_shapes_k2

_RENAME = (("encoder_proj.", "joiner.encoder_proj."), ("decoder_proj.", "joiner.decoder_proj."), ("output_linear.", "joiner.output_linear."))


def _scope(node_name):
    """'/encoder/encoders.0/layers.0/feed_forward1/in_proj/MatMul' -> 'encoder.encoders.0.layers.0.feed_forward1.in_proj'"""
    parts = [p for p in node_name.split("/") if p]
    return ".".join(parts[:-1])


def _canonical(key):
    for a, b in _RENAME:
        if key.startswith(a):
            return b + key[len(a):]
    return key


def _put(sd, seen, key, value):
    """first occurrence wins (the same folded constant may appear at several nodes), a SECOND DIFFERENT value for one key is a
    layout this reader does not understand: refuse instead of loading a wrongly matched constant"""
    seen[key] = seen.get(key, 0) + 1
    if key in sd:
        if tuple(sd[key].shape) != tuple(value.shape) or not torch.equal(sd[key], value):
            raise UnsupportedCheckpoint(f"two different constants in the ONNX graph map to {key!r} (export layout differs from what this reader expects)")
        return
    sd[key] = value


def _collect(model, sd, seen, q=None):
    """q is None: a quantized graph is refused; else its quantize_dynamic chains are read first (`_collect_quantized`)"""
    chain = set()
    if q is None:
        if any(n.op_type in _QUANT_OPS for n in model.nodes):
            raise UnsupportedCheckpoint("a quantized (int8) ONNX graph: only the float32 files are read")
    else:
        chain = _collect_quantized(model, sd, seen, q)
    init = model.initializers
    for name, arr in init.items():
        if re.search(r"\.(weight|bias|bypass_scale)$", name) and arr.dtype == np.float32:
            sd[_canonical(name)] = torch.from_numpy(np.array(arr))
    for n in model.nodes:
        consts = [i for i in n.inputs if i in init]
        if not consts or id(n) in chain or n.op_type in _QUANT_OPS:
            continue
        scope = _canonical(_scope(n.name) + ".")[:-1]
        if n.op_type == "MatMul" and len(n.inputs) == 2 and n.inputs[1] in init and init[n.inputs[1]].ndim == 2:
            _put(sd, seen, scope + ".weight", torch.from_numpy(np.array(init[n.inputs[1]]).T.copy()))
        elif n.op_type == "Gemm" and len(n.inputs) >= 2 and n.inputs[1] in init:
            _put(sd, seen, scope + ".weight", torch.from_numpy(np.array(init[n.inputs[1]])))
            if len(n.inputs) > 2 and n.inputs[2] in init:
                _put(sd, seen, scope + ".bias", torch.from_numpy(np.array(init[n.inputs[2]])))
        elif n.op_type == "Add" and scope + ".weight" in sd:
            c = init[consts[0]]
            if c.ndim == 1 and c.shape[0] == sd[scope + ".weight"].shape[0]:
                _put(sd, seen, scope + ".bias", torch.from_numpy(np.array(c)))
        elif n.op_type == "Mul":
            c = init[consts[0]]
            if (scope.endswith("norm") or scope.endswith("out_norm")) and c.size == 1 and float(c.reshape(-1)[0]) > 0:
                _put(sd, seen, scope + ".log_scale", torch.tensor(math.log(float(c.reshape(-1)[0])), dtype=torch.float32))
            elif (scope.endswith("downsample") or scope.endswith("downsample_output")) and c.ndim >= 1 and c.size in (2, 4, 8) and np.all(c > 0):
                total = float(np.array(c, np.float64).sum())
                if abs(total - 1.0) > 1e-4:
                    raise UnsupportedCheckpoint(f"the constant under {scope!r} sums to {total:.6f}: not a folded softmax(bias) (export layout differs)")
                _put(sd, seen, scope + ".bias", torch.from_numpy(np.log(np.array(c, np.float64).reshape(-1)).astype(np.float32)))


_QUANT_OPS = ("DynamicQuantizeLinear", "MatMulInteger", "QLinearMatMul", "ConvInteger", "DequantizeLinear")


def _scalar(init, name, what, scope):
    if name not in init:
        raise UnsupportedCheckpoint(f"a quantized (int8) MatMul under {scope!r} whose {what} is not a constant: not the quantize_dynamic layout")
    a = np.asarray(init[name])
    if a.size != 1:
        raise UnsupportedCheckpoint(f"a quantized (int8) MatMul under {scope!r} with a per-channel {what} ({a.size} values): only per-tensor "
                                    "quantization (quantize_dynamic's default) is read")
    return a.reshape(-1)[0]


def _collect_quantized(model, sd, seen, q):
    """the quantize_dynamic chains of one file (module docstring), recognised by graph structure: each MatMulInteger must take
    its A operand and zero point from a DynamicQuantizeLinear, a constant int8 B with a per-tensor zero point, and feed a Cast
    whose result is multiplied by Mul(sx, sw) with a per-tensor constant sw.  The Linear is the MatMulInteger's node scope (as
    for a float MatMul); sd receives the dequantized weight (Wq - zw) sw [out][in], q the quantized one.  -> the chain's nodes"""
    for n in model.nodes:
        if n.op_type in ("QLinearMatMul", "ConvInteger", "DequantizeLinear"):
            raise UnsupportedCheckpoint(f"a quantized (int8) ONNX graph with {n.op_type} ({n.name!r}): only quantize_dynamic's "
                                        "DynamicQuantizeLinear + MatMulInteger form is read")
    init = model.initializers
    producer = {o: n for n in model.nodes for o in n.outputs}
    users = {}
    for n in model.nodes:
        for i in n.inputs:
            users.setdefault(i, []).append(n)
    chain = set()
    for n in model.nodes:
        if n.op_type != "MatMulInteger":
            continue
        scope = _canonical(_scope(n.name) + ".")[:-1]
        if len(n.inputs) < 2 or n.inputs[1] not in init or np.asarray(init[n.inputs[1]]).ndim != 2 or init[n.inputs[1]].dtype != np.int8:
            raise UnsupportedCheckpoint(f"a quantized (int8) MatMulInteger under {scope!r} without a constant int8 weight: only MatMuls "
                                        "with a constant B (MatMulConstBOnly) are read")
        if scope.startswith("joiner.decoder_proj") or scope.startswith("joiner.output_linear"):
            raise UnsupportedCheckpoint(f"a quantized (int8) {scope!r}: decoder_proj and output_linear are read as float32 Gemm "
                                        "nodes only (the export squeezes them to 2-D, so quantize_dynamic leaves them float32)")
        dql = producer.get(n.inputs[0])
        if dql is None or dql.op_type != "DynamicQuantizeLinear" or len(dql.outputs) < 3 or len(n.inputs) < 3 or n.inputs[2] != dql.outputs[2]:
            raise UnsupportedCheckpoint(f"a quantized (int8) MatMulInteger under {scope!r} whose activation does not come from a "
                                        "DynamicQuantizeLinear: not the quantize_dynamic layout")
        zw = int(_scalar(init, n.inputs[3], "weight zero point", scope)) if len(n.inputs) > 3 and n.inputs[3] else 0
        cast = [u for u in users.get(n.outputs[0], []) if u.op_type == "Cast"]
        muls = [u for u in users.get(cast[0].outputs[0], []) if u.op_type == "Mul"] if len(cast) == 1 else []
        sw = None
        for m in muls:
            other = [i for i in m.inputs if i != cast[0].outputs[0]]
            sm = producer.get(other[0]) if len(other) == 1 else None
            if sm is not None and sm.op_type == "Mul" and dql.outputs[1] in sm.inputs:
                sw_name = [i for i in sm.inputs if i != dql.outputs[1]]
                if len(sw_name) == 1:
                    sw = float(np.float32(_scalar(init, sw_name[0], "weight scale", scope)))
                    chain.update((id(m), id(sm)))
                    break
        if sw is None:
            raise UnsupportedCheckpoint(f"a quantized (int8) MatMulInteger under {scope!r} without its scale Mul(Cast(.), Mul(sx, sw)): "
                                        "not the quantize_dynamic layout")
        wq = np.ascontiguousarray(np.asarray(init[n.inputs[1]]).T)                         # [out][in]
        deq = (wq.astype(np.float32) - np.float32(zw)) * np.float32(sw)
        _put(sd, seen, scope + ".weight", torch.from_numpy(deq))
        if scope in q:
            raise UnsupportedCheckpoint(f"two quantized MatMuls map to {scope!r} (export layout differs from what this reader expects)")
        q[scope] = (torch.from_numpy(wq), sw, zw)
        chain.update((id(n), id(dql), id(cast[0])))
    return chain


def derive_config(sd) -> ZipformerConfig:
    """ZipformerConfig from the shapes of an icefall-style state dict"""
    def shape(k):
        if k not in sd:
            raise UnsupportedCheckpoint(f"the ONNX files hold no tensor that maps to {k!r} (export layout differs from what this reader expects)")
        return tuple(sd[k].shape)
    c1 = shape("encoder_embed.conv.0.weight")[0]
    c2 = shape("encoder_embed.conv.4.weight")[0]
    c3 = shape("encoder_embed.conv.7.weight")[0]
    stacks = sorted({int(m.group(1)) for k in sd for m in [re.match(r"encoder\.encoders\.(\d+)\.", k)] if m})
    dims, layers, ffs, heads, kernels, dss = [], [], [], [], [], []
    for s in stacks:
        down = f"encoder.encoders.{s}.downsample.bias" in sd
        base = f"encoder.encoders.{s}." + ("encoder." if down else "") + "layers."
        n = 1 + max(int(m.group(1)) for k in sd for m in [re.match(re.escape(base) + r"(\d+)\.", k)] if m)
        L = base + "0."
        d = shape(L + "feed_forward2.in_proj.weight")[1]
        dims.append(d); layers.append(n)
        ffs.append(shape(L + "feed_forward2.in_proj.weight")[0])
        heads.append(shape(L + "self_attn1.in_proj.weight")[0] // 12)
        kernels.append(shape(L + "conv_module1.depthwise_conv.weight")[-1])
        dss.append(int(sd[f"encoder.encoders.{s}.downsample.bias"].numel()) if down else 1)
    h0 = heads[0]
    in_proj = shape(layer_prefix_from(dss, 0) + "self_attn_weights.in_proj.weight")[0]
    pos_w = shape(layer_prefix_from(dss, 0) + "self_attn_weights.linear_pos.weight")
    pd = pos_w[0] // h0
    qd = (in_proj // h0 - pd) // 2
    V, D = shape("decoder.embedding.weight")
    return ZipformerConfig(embed_channels=(c1, c2, c3), encoder_dim=tuple(dims), num_layers=tuple(layers), ff_dim=tuple(ffs), num_heads=tuple(heads),
                           cnn_kernel=tuple(kernels), downsampling=tuple(dss), query_head_dim=qd, value_head_dim=12, pos_head_dim=pd, pos_dim=pos_w[1],
                           vocab_size=V, decoder_dim=D, joiner_dim=shape("joiner.output_linear.weight")[1],
                           context_size=shape("decoder.conv.weight")[-1]).validate()


def layer_prefix_from(dss, s):
    return f"encoder.encoders.{s}." + ("" if dss[s] == 1 else "encoder.") + "layers.0."


def self_check(cfg, sd):
    """what a wrongly matched constant cannot survive: the recovered keys are EXACTLY the keys of an icefall Zipformer2 transducer
    of the derived architecture, every shape agrees, the parameter count equals cfg.n_params(), BiasNorm log-scales and bypass
    scales are finite and in the range training keeps them in ([UPSTREAM] scaling.py: log_scale limited to +-1.5, bypass_scale
    to [0, 1] with slack)."""
    want = expected_shapes_k2(cfg)
    missing, extra = sorted(set(want) - set(sd)), sorted(set(sd) - set(want))
    if missing or extra:
        raise UnsupportedCheckpoint(f"the ONNX files do not map onto an icefall Zipformer2 transducer of the derived architecture: "
                                    f"{len(missing)} tensor(s) not found ({', '.join(missing[:4])}{' ...' if len(missing) > 4 else ''}), "
                                    f"{len(extra)} unexpected ({', '.join(extra[:4])}{' ...' if len(extra) > 4 else ''})")
    for k, shp in want.items():
        if tuple(sd[k].shape) != shp:
            raise UnsupportedCheckpoint(f"tensor {k!r} has shape {tuple(sd[k].shape)}, the derived architecture needs {shp}")
        if not bool(torch.isfinite(sd[k]).all()):
            raise UnsupportedCheckpoint(f"tensor {k!r} holds non-finite values")
    n = sum(int(v.numel()) for v in sd.values())
    if n != cfg.n_params():
        raise UnsupportedCheckpoint(f"{n} parameters recovered, the derived architecture has {cfg.n_params()}")
    for k, v in sd.items():
        if k.endswith(".log_scale") and abs(float(v)) > 4.0:
            raise UnsupportedCheckpoint(f"{k!r} = {float(v):.3f}: not a BiasNorm log-scale (a wrongly matched Mul constant?)")
        if k.endswith(".bypass_scale") and (float(v.min()) < -0.5 or float(v.max()) > 1.5):
            raise UnsupportedCheckpoint(f"{k!r} outside [-0.5, 1.5]: not a bypass scale")


def read_k2_onnx(encoder_path, decoder_path, joiner_path):
    """-> (ZipformerConfig, icefall-style state dict), checked by `self_check`.  UNVERIFIED against a real export (module
    docstring): compare one transcript with sherpa-onnx before trusting a first real checkpoint."""
    sd, seen = {}, {}
    for path in (encoder_path, decoder_path, joiner_path):
        _collect(onnx_lite.load(path), sd, seen)
    cfg = derive_config(sd)
    self_check(cfg, sd)
    return cfg, sd


def read_k2_onnx_quantized(encoder_path, decoder_path, joiner_path):
    """the "int8" / "int8-fp32" files (module docstring) -> (ZipformerConfig, state dict, q): the state dict holds the dequantized
    float32 weights (Wq - zw) sw of the quantized Linears, so `derive_config` and `self_check` run unchanged; q maps every quantized
    Linear (icefall name) to (Wq int8 [out][in], sw, zw).  Refused with "quantized" in the message: MatMulInteger with a
    non-constant B, a per-channel scale or zero point, a chain without its scale Mul, QLinearMatMul / ConvInteger /
    DequantizeLinear, and a quantized decoder_proj / output_linear (a deliberate limit: the export is expected to leave them
    float32 Gemm nodes).  UNVERIFIED against a real export, like `read_k2_onnx`."""
    sd, seen, q = {}, {}, {}
    for path in (encoder_path, decoder_path, joiner_path):
        _collect(onnx_lite.load(path), sd, seen, q)
    cfg = derive_config(sd)
    self_check(cfg, sd)
    if not q:
        raise UnsupportedCheckpoint("no quantized (int8) MatMul found: these are float32 files (read them with precision='fp32')")
    return cfg, sd, q
