"""Same-process A/B of the three kernels in front of the first encoder layer, each against its first form (RS_LOGMEL_OLD,
RS_SUB_CONV0_OLD, RS_SUB_DW_OLD of csrc/rs_knobs.h), at the bench's shapes: 256 x 10 s (+ 0.5 s pad each side), sub_channels 256.

    python scripts/front_forms_ab.py [--reps 5] [--iters 10] [--batch 256] [--seconds 10]

The encoder is the shipped configuration cut to ONE layer (the front of the encoder does not depend on the depth).  Times are
HIP-event brackets of the launchers (rs_profile_enable): PROF_FRONTEND = logmel_kernel + feat_normalize_kernel, PROF_SUBSAMPLE =
sub_conv0_dw1 + sub_dw; one switch changes between two neighbouring measurements, so the difference is the kernel's.  Forms are
interleaved: rep r runs new, old, new, old ... of every switch.  Printed per switch: every repetition's ms per step of its class,
the means, the gap and the spread (max - min) of the first form's repetitions — a form counts as faster only if the gap exceeds
that spread.  The log-mel switch is also measured on the ESPnet (kind 1) and Zipformer (kind 2) front ends.
"""
import argparse
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from reazonspeech_amd.runtime import capi  # noqa: E402
from reazonspeech_amd.runtime.config import ESPNET_CONFORMER_120M, FASTCONFORMER_619M  # noqa: E402
from reazonspeech_amd.runtime.k2_config import ZIPFORMER_159M  # noqa: E402
from reazonspeech_amd.runtime.k2_weights import synthetic_state_dict_k2  # noqa: E402
from reazonspeech_amd.runtime.model import AsrModel  # noqa: E402
from reazonspeech_amd.runtime.synth import synthetic_batch  # noqa: E402
from reazonspeech_amd.runtime.weights import synthetic_state_dict  # noqa: E402
from reazonspeech_amd.runtime.weights_espnet import synthetic_state_dict_espnet  # noqa: E402


def set_knob(lib, name, value):
    lib.rs_debug_set_knob.argtypes = [ctypes.c_char_p, ctypes.c_int]
    lib.rs_debug_set_knob.restype = ctypes.c_int
    assert lib.rs_debug_set_knob(name.encode(), int(value)) == 0, name


def measure(model, buf, klass, iters, encoder):
    """ms per step of the profiled class over `iters` front-end (+ encoder) passes"""
    ctx = model.ctx
    with torch.cuda.device(model.device):
        stream = torch.cuda.current_stream().cuda_stream
        ctx.profile_reset()
        ctx.profile_enable(klass)
        for _ in range(iters):
            ctx.frontend(buf.audio, buf.lens, model.pad_left, model.pad_right, buf.t_max, buf.feats, buf.n_frames, buf.ws, stream)
            if encoder:
                ctx.encoder(buf.feats, buf.n_frames, buf.B, buf.t_max, None, buf.joint_enc, buf.enc_lens, buf.ws, stream)
        torch.cuda.synchronize()
        got = ctx.profile_read(klass)
        ctx.profile_enable(0)
    return got["ms"] / iters


def ab(model, buf, switch, klass, reps, iters, encoder, label):
    lib = model.ctx.lib
    new, old = [], []
    measure(model, buf, klass, 2, encoder)                    # warm-up
    for _ in range(reps):
        set_knob(lib, switch, 0)
        new.append(measure(model, buf, klass, iters, encoder))
        set_knob(lib, switch, 1)
        old.append(measure(model, buf, klass, iters, encoder))
    set_knob(lib, switch, 0)
    mean_new, mean_old = sum(new) / reps, sum(old) / reps
    spread = max(old) - min(old)
    gap = mean_old - mean_new
    print(f"{label} {switch}: class ms per step, {reps} interleaved repetitions of {iters} steps")
    print("   new  " + " ".join(f"{x:.4f}" for x in new) + f"   mean {mean_new:.4f}")
    print("   old  " + " ".join(f"{x:.4f}" for x in old) + f"   mean {mean_old:.4f}   spread {spread:.4f}")
    print(f"   gap {gap * 1e3:+.1f} us ({'faster' if gap > spread else 'NOT faster'}: gap {'>' if gap > spread else '<='} spread of the first form)", flush=True)


def staged(model, batch, seconds, seed):
    audio, lens = synthetic_batch(batch, seconds, seed=seed)
    buf = model.stage([audio[i, :lens[i]] for i in range(batch)], buf=model.new_buffers(batch, int(seconds * 16000)))
    torch.cuda.synchronize()
    return buf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=10.0)
    args = ap.parse_args()

    cfg = FASTCONFORMER_619M.with_(n_layers=1)
    model = AsrModel(cfg, synthetic_state_dict(cfg, seed=0), None, device="cuda:0")
    buf = staged(model, args.batch, args.seconds, 1234)
    print(f"nemo: B = {buf.B}, t_max = {buf.t_max}, sub_channels = {cfg.sub_channels}")
    ab(model, buf, "RS_LOGMEL_OLD", capi.PROF_FRONTEND, args.reps, args.iters, False, "nemo (kind 0)")
    ab(model, buf, "RS_SUB_CONV0_OLD", capi.PROF_SUBSAMPLE, args.reps, args.iters, True, "nemo")
    ab(model, buf, "RS_SUB_DW_OLD", capi.PROF_SUBSAMPLE, args.reps, args.iters, True, "nemo")
    del model, buf

    cfg = ESPNET_CONFORMER_120M.with_(n_layers=1)
    model = AsrModel(cfg, synthetic_state_dict_espnet(cfg, 0), None, device="cuda:0")
    buf = staged(model, args.batch, args.seconds, 1234)
    ab(model, buf, "RS_LOGMEL_OLD", capi.PROF_FRONTEND, args.reps, args.iters, False, f"espnet (kind 1, t_max = {buf.t_max})")
    del model, buf

    cfg = ZIPFORMER_159M
    model = AsrModel(cfg, synthetic_state_dict_k2(cfg, 0), None, device="cuda:0")
    buf = staged(model, args.batch, args.seconds, 1234)
    ab(model, buf, "RS_LOGMEL_OLD", capi.PROF_FRONTEND, args.reps, args.iters, False, f"k2 (kind 2, t_max = {buf.t_max})")


if __name__ == "__main__":
    main()
