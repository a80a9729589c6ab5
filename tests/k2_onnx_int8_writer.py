"""Test-only writer of the "int8" / "int8-fp32" ONNX files in the layout `runtime/k2_onnx.py: read_k2_onnx_quantized` is written
for: the float files of `k2_onnx_writer.write_k2_onnx`, with every MatMul of the encoder file whose B operand is a constant rewritten
the way onnxruntime's quantize_dynamic(op_types_to_quantize=["MatMul"], weight_type=QInt8) does ([UPSTREAM], see the reader's
module docstring):
    DynamicQuantizeLinear(x) -> (xq, sx, zx);  MatMulInteger(xq, Wq, zx, zw);  Cast;  Mul(., Mul(sx, sw))
with ORT-style names (initializers "<weight>_quantized" / "_scale" / "_zero_point", nodes "<MatMul>_quant" ...).  The weights come
from `quantize_k2_linears` (or any {name: (Wq, sw, zw)}).  NOT an onnxruntime output: a stand-in with the documented structure."""
import numpy as np

from k2_onnx_writer import write_k2_onnx
from reazonspeech_amd.runtime import onnx_lite, k2_onnx


def quantize_matmuls(model, q, only=None):
    """rewrite, in place, every MatMul whose scope maps to a Linear of q (and of `only`, when given) into the quantize_dynamic chain"""
    nodes = []
    for n in model.nodes:
        key = k2_onnx._canonical(k2_onnx._scope(n.name) + ".")[:-1]
        if n.op_type != "MatMul" or key not in q or (only is not None and key not in only):
            nodes.append(n)
            continue
        wq, sw, zw = q[key]
        wname = n.inputs[1]
        del model.initializers[wname]
        model.initializers[wname + "_quantized"] = np.ascontiguousarray(wq.numpy().T)          # [K][N]
        model.initializers[wname + "_scale"] = np.asarray(sw, np.float32)
        model.initializers[wname + "_zero_point"] = np.asarray(zw, np.int8)
        x, t = n.inputs[0], n.name
        xq, sx, zx = t + "/xq", t + "/sx", t + "/zx"
        nodes += [
            onnx_lite.Node(x + "_QuantizeLinear", "DynamicQuantizeLinear", [x], [xq, sx, zx]),
            onnx_lite.Node(t + "_quant", "MatMulInteger", [xq, wname + "_quantized", zx, wname + "_zero_point"], [t + "/i32"]),
            onnx_lite.Node(t + "_output_quantized_cast", "Cast", [t + "/i32"], [t + "/f32"]),
            onnx_lite.Node(t + "_scales_mul", "Mul", [sx, wname + "_scale"], [t + "/scale"]),
            onnx_lite.Node(t + "_output_scale_mul", "Mul", [t + "/f32", t + "/scale"], n.outputs),
        ]
    model.nodes = nodes
    return model


def write_k2_onnx_int8(cfg, sd, q, encoder_path, decoder_path, joiner_path):
    """the three files of the "int8" set (decoder and joiner hold no quantized MatMul: decoder_proj / output_linear are Gemm nodes
    in a real export); for "int8-fp32" pass the float decoder file's path as decoder_path — its content is the same"""
    write_k2_onnx(cfg, sd, encoder_path, decoder_path, joiner_path)
    m = onnx_lite.load(encoder_path)
    onnx_lite.dump(encoder_path, quantize_matmuls(m, q))
