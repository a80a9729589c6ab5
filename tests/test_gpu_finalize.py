"""-m gpu: what rs_finalize accepts and refuses, for all four families (no kernel is launched: the tensors only have to be on
the device, and every case is a fresh context over the same uploaded tensors).

Each family's own prepared tensors (prepare_weights*, the toy configurations of the other suites) are registered on a fresh
capi.Context.  The complete set finalizes; a tensor left out is RS_EMISSING and the text names it; a tensor a few elements short
is RS_EINVAL and the text names it with the size that was expected; a tensor registered from a view 8 bytes into an allocation
is RS_EINVAL.  The optional groups: the screened joint's four tensors are all there or none; the Zipformer's float32 set is
complete once "emb.out.w.f32" is there; a quantized Linear is its three tensors.  With several tensors wrong, the error is that
of the first lookup in the library's order: the bf16 model from the front-end to the joiner, then the screened joint, then the
float32 set (encoder_embed, joiner.encoder_proj, the stacks), then the int8 one."""
import pytest
import torch

from reazonspeech_amd.runtime import capi
from reazonspeech_amd.runtime.avsr_config import AVSR_TINY
from reazonspeech_amd.runtime.avsr_weights import prepare_weights_avsr, synthetic_state_dict_avsr
from reazonspeech_amd.runtime.config import ESPNET_TINY, TINY
from reazonspeech_amd.runtime.k2_config import ZIPFORMER_TINY
from reazonspeech_amd.runtime import k2_weights as kw
from reazonspeech_amd.runtime.weights import prepare_weights, synthetic_state_dict
from reazonspeech_amd.runtime.weights_espnet import prepare_weights_espnet, synthetic_state_dict_espnet

pytestmark = pytest.mark.gpu
RS_EINVAL, RS_EMISSING = -1, -2
POS_CAP = 64
SCREEN = ("joint.out.w16", "joint.out.wrm", "joint.out.bpad", "joint.out.wmax")

# a dense weight and a float32 vector from the middle of each model
PROBES = [("nemo", "L1.ff2.w2"), ("nemo", "L0.ln_conv.g"), ("espnet", "L1.att.qkv.w"), ("espnet", "ctc.b"),
          ("k2", "S1.L0.na.out.w"), ("k2", "S1.L0.cm2.dw.b"), ("avsr", "D0.ca.kv.w"), ("avsr", "v.l3.0.ds.bn.alpha")]


def _k2_tensors():
    cfg = ZIPFORMER_TINY
    sd = kw.synthetic_state_dict_k2(cfg, 3)
    q = kw.quantize_k2_linears(cfg, sd)
    return kw.prepare_weights_k2(cfg, kw.dequantize_k2_linears(sd, q), POS_CAP, f32=True, i8=q)


@pytest.fixture(scope="module")
def families(gpu_device):
    """family -> (configuration, {name: tensor on the device}): the complete set, every optional group included"""
    host = {"nemo": (TINY, prepare_weights(TINY, synthetic_state_dict(TINY, 5), POS_CAP, f32=True)),
            "espnet": (ESPNET_TINY, prepare_weights_espnet(ESPNET_TINY, synthetic_state_dict_espnet(ESPNET_TINY, 3), POS_CAP, f32=True)),
            "k2": (ZIPFORMER_TINY, _k2_tensors()),
            "avsr": (AVSR_TINY, prepare_weights_avsr(AVSR_TINY, synthetic_state_dict_avsr(AVSR_TINY, 3)))}
    return {f: (cfg, {n: t.to(gpu_device).contiguous() for n, t in ts.items()}) for f, (cfg, ts) in host.items()}


def finalize(families, family, drop=(), replace=None):
    """a fresh context over the family's tensors without `drop` and with `replace` = {name: tensor} in place of its own"""
    cfg, tensors = families[family]
    for name in list(drop) + list(replace or {}):
        assert name in tensors, name
    ctx = capi.Context(cfg, 0)
    try:
        for name, t in tensors.items():
            if name not in drop:
                ctx.set_tensor(name, (replace or {}).get(name, t))
        ctx.finalize()
    finally:
        ctx.close()


def refused(families, family, **kw):
    with pytest.raises(capi.RsError) as e:
        finalize(families, family, **kw)
    return e.value.code, str(e.value)


def missing(families, family, drop, name):
    code, text = refused(families, family, drop=drop)
    assert code == RS_EMISSING and f"weight tensor '{name}' was not registered" in text, text


@pytest.mark.parametrize("family", ["nemo", "espnet", "k2", "avsr"])
def test_complete_set_finalizes(families, family):
    finalize(families, family)


@pytest.mark.parametrize("family,name", PROBES)
def test_left_out(families, family, name):
    missing(families, family, [name], name)


@pytest.mark.parametrize("family,name", PROBES)
def test_a_few_elements_short(families, family, name):
    t = families[family][1][name]
    short = t.reshape(-1)[:-3]
    code, text = refused(families, family, replace={name: short})
    want, got = t.numel() * t.element_size(), short.numel() * t.element_size()
    assert code == RS_EINVAL and f"tensor '{name}': expected {want} bytes, got {got}" in text, text


@pytest.mark.parametrize("family,name", PROBES)
def test_eight_bytes_into_an_allocation(families, family, name):
    t = families[family][1][name]
    off = 8 // t.element_size()
    room = torch.zeros(t.numel() + 2 * off, dtype=t.dtype, device=t.device)
    assert room.data_ptr() % 16 == 0
    view = room[off:off + t.numel()]
    view.copy_(t.reshape(-1))
    assert view.data_ptr() % 16 == 8 and view.is_contiguous()
    code, text = refused(families, family, replace={name: view})
    assert code == RS_EINVAL and f"tensor '{name}' is not 16-byte aligned" in text, text


@pytest.mark.parametrize("family", ["nemo", "k2"])
@pytest.mark.parametrize("fourth", SCREEN)
def test_screened_joint_is_all_four(families, family, fourth):
    missing(families, family, [fourth], fourth)


@pytest.mark.parametrize("family", ["nemo", "k2"])
def test_screened_joint_may_be_absent(families, family):
    finalize(families, family, drop=SCREEN)


def test_nemo_position_table_is_required(families):
    missing(families, "nemo", ["pos.table"], "pos.table")
    missing(families, "nemo", ["pos.table.f32"], "pos.table.f32")


def test_k2_float32_set_is_complete_or_absent(families):
    missing(families, "k2", ["S0.L0.ff2.out.w.f32"], "S0.L0.ff2.out.w.f32")
    missing(families, "k2", ["S1.L0.cm1.in.b.f32"], "S1.L0.cm1.in.b.f32")
    tensors = families["k2"][1]
    finalize(families, "k2", drop=[n for n in tensors if n.endswith(".f32")])


def test_k2_quantized_linear_is_three_tensors(families):
    missing(families, "k2", ["S0.L0.ff1.in.w.i8.cs"], "S0.L0.ff1.in.w.i8.cs")
    missing(families, "k2", ["S1.L1.attw.pos.w.i8.q"], "S1.L1.attw.pos.w.i8.q")
    missing(families, "k2", ["pos.enc"], "pos.enc")
    # each Linear on its own: one that is not quantized at all is no error
    finalize(families, "k2", drop=["S0.L0.ff1.in.w.i8", "S0.L0.ff1.in.w.i8.cs", "S0.L0.ff1.in.w.i8.q"])


@pytest.mark.parametrize("drop,name", [
    (["emb.conv0.w", "S0.L0.ff1.in.w"], "emb.conv0.w"),
    (["emb.conv0.w", "emb.conv2.w.f32", "emb.out.w.i8.q"], "emb.conv0.w"),
    (["S2.L0.sa2.out.b", "S1.L1.sa1.in.w"], "S1.L1.sa1.in.w"),
    # the table whose size gives the capacity is read between encoder_embed and the stacks
    (["S0.L0.attw.pos_proj", "emb.norm.scale"], "emb.norm.scale"),
    (["S0.L0.attw.pos_proj", "S0.L0.attw.in.w"], "S0.L0.attw.pos_proj"),
    # the whole bf16 model and the screened joint come before the float32 set, and that before the int8 one
    (["joint.out.b", "emb.conv2.w.f32"], "joint.out.b"),
    (["joint.out.wmax", "emb.conv2.w.f32"], "joint.out.wmax"),
    (["S1.L1.na.out.w.f32", "emb.out.w.i8.cs"], "S1.L1.na.out.w.f32"),
    # joiner.encoder_proj: last of the bf16 encoder, but ahead of the stacks in the float32 and int8 sets
    (["joint.enc.w", "out.ds.w"], "out.ds.w"),
    (["joint.enc.w.f32", "S0.L0.attw.in.w.f32"], "joint.enc.w.f32"),
    (["joint.enc.w.i8.cs", "S0.L0.attw.in.w.i8.cs"], "joint.enc.w.i8.cs"),
    (["pos.enc", "S1.L1.na.out.w.i8.q"], "S1.L1.na.out.w.i8.q"),
])
def test_k2_first_failing_lookup_is_reported(families, drop, name):
    missing(families, "k2", drop, name)


def test_nemo_first_failing_lookup_is_reported(families):
    missing(families, "nemo", ["fe.fb_w", "L1.ff1.b1"], "fe.fb_w")
    missing(families, "nemo", ["joint.out.b", "joint.out.w16"], "joint.out.b")
    missing(families, "nemo", ["joint.out.wrm", "L0.ff1.w1.f32"], "joint.out.wrm")
    missing(families, "nemo", ["L1.att.pos.w.f32", "pos.table.f32", "pos.table"], "L1.att.pos.w.f32")
