"""GPU: the family guard at every exported function that takes a context (reazonspeech_amd/csrc/rs_family.h).

Three tiny contexts, one per family, none finalized and without a single registered tensor; no call in this file may get as far as
a launch.  Every row of the table is called on every family:

  a family the row does not serve   RS_EINVAL and "<entry>: not defined for <a family> context" in rs_last_error; a query (a size or
                                    a frame count) answers 0 and leaves the context's text alone
  a family it serves, FINAL row     RS_ESTATE and "rs_finalize must precede <entry>"; a query answers 0
  a family it serves, ANYTIME row   past the guard: the entry's own argument check answers (never RS_ESTATE, no guard text); a query
                                    with arguments that make sense answers with a size

The calls pass NULL for every pointer and 0 for every number unless ARGS below says otherwise, so an entry that got past a wrong
guard would fail its own argument check, not launch.  rs_set_option is checked key by key against the families it names.
(rs_mel_frames / rs_workspace_bytes on an AV-HuBERT context divided by a hop length of 0 before the guard, rs_encoder_forward on one
threw through the C frame, rs_relpos_attention_f32 on a Zipformer or AV-HuBERT context divided by a head count of 0.)"""
import ctypes
import os
import re

import pytest

from reazonspeech_amd.runtime import capi
from reazonspeech_amd.runtime.avsr_config import AVSR_TINY
from reazonspeech_amd.runtime.config import TINY
from reazonspeech_amd.runtime.k2_config import ZIPFORMER_TINY

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RS_OK, RS_EINVAL, RS_EMISSING, RS_ESTATE = 0, -1, -2, -6
FAMILIES = {"C": ("a Conformer", TINY), "Z": ("a Zipformer", ZIPFORMER_TINY), "A": ("an AV-HuBERT", AVSR_TINY)}
SERVES = {"ALL": "CZA", "CZ": "CZ", "C": "C", "Z": "Z", "A": "A"}
MARK = "unknown option '__mark__'"

# arguments after the context for the queries that answer with a size on a family they serve (everything else: zeros and NULLs)
ARGS = {
    "rs_workspace_bytes": (1, 16000), "rs_mel_frames": (16000,), "rs_enc_frames": (100,),
    "rs_rnnt_alsd_workspace_bytes": (1, 2, 10, 1.0, -1), "rs_rnnt_beam_workspace_bytes": (1, 2, 10, 0),
    "rs_rnnt_mbs_workspace_bytes": (1, 4, 10, 10), "rs_rnnt_mbs_hotwords_workspace_bytes": (1, 4, 10, 10),
    "rs_rnnt_token_scores_workspace_bytes": (1, 8), "rs_ctc_align_workspace_bytes": (1, 10, 4, 2),
    "rs_avsr_workspace_bytes": (1, 4), "rs_avsr_decoder_state_bytes": (1, 4, 2, 8),
    "rs_avsr_search_state_bytes": (1, 2, 8), "rs_avsr_search_state_bytes_opts": (1, 2, 8, 16, None), "rs_avsr_search_state_bytes_scored": (1, 2, 8, 16, None),
    "rs_avsr_generate_state_bytes": (1, 4, 2, 8), "rs_avsr_generate_state_bytes_opts": (1, 4, 2, 8, None),
    "rs_avsr_generate_state_bytes_scored": (1, 4, 2, 8, None),
}
OPTIONS = {"decode_screen": "CZ", "decode_narrow": "CZ", "precision_f32": "CZ", "precision_i8": "Z", "gemm_f32_x3": "CZA", "k2_conv2_fused": "Z",
           "k2_cnx_fused": "Z", "fuse_glu": "C", "defer_out_norm": "C"}


def table():
    """[(entry, families served as letters, needs finalize)] from the X-macro rows"""
    text = open(os.path.join(ROOT, "reazonspeech_amd", "csrc", "rs_family.h")).read()
    rows = re.findall(r"^\s*X\((rs_\w+), (ALL|CZ|C|Z|A), (ANYTIME|FINAL), ", text, flags=re.M)
    assert len(rows) >= 60 and len({r[0] for r in rows}) == len(rows)
    return [(name, SERVES[serves], when == "FINAL") for name, serves, when in rows]


def queries():
    """the entries whose context is const: sizes and frame counts (0 on a refusal, no text), and rs_last_error"""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rs_asr.h")).read(), flags=re.S)
    return set(re.findall(r"\b(rs_[a-z0-9_]+)\s*\(\s*const\s+rs_ctx\s*\*", src))


@pytest.fixture(scope="module")
def contexts(gpu_device):
    made = {letter: capi.Context(cfg, 0) for letter, (_, cfg) in FAMILIES.items()}
    yield made
    for c in made.values():
        c.close()


def zero(argtype):
    if argtype in (ctypes.c_float, ctypes.c_double):
        return 0.0
    if argtype in (ctypes.c_int, ctypes.c_int32, ctypes.c_int64, ctypes.c_size_t):
        return 0
    return None                                           # every kind of pointer, the option key included


def call(ctx, name):
    """entry `name` on `ctx` -> (what it returned, the context's text afterwards); the text is set to MARK first"""
    lib = ctx.lib
    assert lib.rs_set_option(ctx._h, b"__mark__", 0) == RS_EINVAL and lib.rs_last_error(ctx._h).decode() == MARK
    fn = getattr(lib, name)
    args = ARGS.get(name) or tuple(zero(t) for t in fn.argtypes[1:])
    assert len(args) == len(fn.argtypes) - 1, name
    got = fn(ctx._h, *args)
    return got, lib.rs_last_error(ctx._h).decode()


def test_every_row_on_every_family(contexts):
    const = queries()
    assert {"rs_mel_frames", "rs_enc_frames", "rs_workspace_bytes", "rs_avsr_workspace_bytes"} <= const
    wrong = served = 0
    for name, serves, final in table():
        if name in ("rs_destroy", "rs_last_error"):       # every family, any time: the fixture and every other call use them
            assert serves == "CZA" and not final
            continue
        for letter, (family, _) in FAMILIES.items():
            got, text = call(contexts[letter], name)
            where = (name, letter, got, text)
            if letter not in serves:
                wrong += 1
                if name in const:
                    assert got == 0 and text == MARK, where
                else:
                    assert got == RS_EINVAL and f"{name}: not defined for {family} context" in text, where
                continue
            served += 1
            if final:
                if name in const:
                    assert got == 0 and text == MARK, where
                else:
                    assert got == RS_ESTATE and text == f"rs_finalize must precede {name}", where
            elif name in const:
                assert got > 0 and text == MARK, where    # the same arguments answer 0 on a family the row does not serve
            else:
                assert got in (RS_OK, RS_EINVAL, RS_EMISSING) and "not defined for" not in text and "must precede" not in text, where
                assert got != RS_OK or text == MARK, where
    assert wrong >= 80 and served >= 100, (wrong, served)


def test_the_calls_that_went_wrong_before_the_guard(contexts):
    avsr, k2 = contexts["A"], contexts["Z"]
    assert avsr.mel_frames(16000) == 0 and avsr.workspace_bytes(4, 16000) == 0 and avsr.enc_frames(100) == 0
    for ctx, family in ((avsr, "an AV-HuBERT"), (k2, "a Zipformer")):
        got, text = call(ctx, "rs_relpos_attention_f32")
        assert got == RS_EINVAL and f"rs_relpos_attention_f32: not defined for {family} context" in text
    got, text = call(avsr, "rs_encoder_forward")
    assert got == RS_EINVAL and "rs_encoder_forward: not defined for an AV-HuBERT context" in text and "rs_avsr_encoder_forward" in text
    # the taps, crosswise: each family's own entry answers, the other two are refused and say where to go
    taps = {"C": "rs_encoder_set_taps", "Z": "rs_k2_encoder_set_taps", "A": "rs_avsr_encoder_set_taps"}
    for owner, entry in taps.items():
        for letter, (family, _) in FAMILIES.items():
            got, text = call(contexts[letter], entry)
            if letter == owner:
                assert got == RS_OK and text == MARK, (entry, letter, got, text)
            else:
                assert got == RS_EINVAL and f"{entry}: not defined for {family} context" in text and taps[letter] in text, (entry, letter, got, text)
    # a wrong pairing is refused without any weights: the family test comes before the finalized test
    got, text = call(k2, "rs_rnnt_alsd")
    assert got == RS_EINVAL and "rs_rnnt_alsd: not defined for a Zipformer context" in text and "stateless decoder; only rs_rnnt_greedy applies" in text
    got, text = call(contexts["C"], "rs_rnnt_mbs")
    assert got == RS_EINVAL and "rs_rnnt_mbs: not defined for a Conformer context" in text and "Zipformer" in text


def test_set_option_key_by_key(contexts):
    for key, serves in OPTIONS.items():
        for letter, (family, _) in FAMILIES.items():
            ctx = contexts[letter]
            ctx.lib.rs_set_option(ctx._h, b"__mark__", 0)
            rc = ctx.lib.rs_set_option(ctx._h, key.encode(), 0)       # 0: no key needs registered tensors to be switched off
            text = ctx.lib.rs_last_error(ctx._h).decode()
            if letter in serves:
                assert rc == RS_OK and text == MARK, (key, letter, rc, text)
            else:
                assert rc == RS_EINVAL and "rs_set_option" in text and f"'{key}'" in text and f"does not apply to {family} context" in text, (key, letter, rc, text)
    for ctx in contexts.values():
        assert ctx.lib.rs_set_option(ctx._h, b"no_such_option", 1) == RS_EINVAL and "unknown option 'no_such_option'" in ctx.lib.rs_last_error(ctx._h).decode()
        assert ctx.lib.rs_set_option(ctx._h, None, 1) == RS_EINVAL
    c = contexts["C"]
    assert c.lib.rs_set_option(c._h, b"fuse_glu", 2) == RS_EINVAL and "fuse_glu must be 0 or 1" in c.lib.rs_last_error(c._h).decode()
    for key in ("fuse_glu", "defer_out_norm", "decode_screen", "decode_narrow"):          # back to the defaults
        assert c.lib.rs_set_option(c._h, key.encode(), 1) == RS_OK


def test_null_context():
    lib = capi.load()
    const = queries()
    for name, _, _ in table():
        if name == "rs_destroy":
            lib.rs_destroy(None)
            continue
        fn = getattr(lib, name)
        got = fn(None, *(ARGS.get(name) or tuple(zero(t) for t in fn.argtypes[1:])))
        if name == "rs_last_error":
            assert got == b"null context"
        else:
            assert got == (0 if name in const else RS_EINVAL), (name, got)
