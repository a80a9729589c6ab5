"""CPU: the family table and its guard (reazonspeech_amd/csrc/rs_family.h).

A stand-alone program (tests/family_host_main.cpp) is built from the header alone with g++ -Wall -Werror, once plain and once under
AddressSanitizer + UBSan.  The table must have exactly one row per function of include/rs_asr.h that takes a context; the guard must
refuse in the order null context (RS_EINVAL), family (RS_EINVAL), not finalized (RS_ESTATE) for every combination; every refusal
names its entry, a family refusal the family too.  The source checks keep the guard the first statement of every such function and
the guard the only place in csrc/ that asks which family a context is."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "reazonspeech_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "rs_asr.h")
MAIN = os.path.join(ROOT, "tests", "family_host_main.cpp")
RS_OK, RS_EINVAL, RS_ESTATE = 0, -1, -6
FAMILIES = {0: "a Conformer", 1: "a Zipformer", 2: "an AV-HuBERT"}


def declared_entries():
    """{function: (return type, the context is const)} of every function the header declares whose first parameter is the context.
    The const ones are the queries: a size or a frame count, 0 on a refusal and no message (rs_last_error: its fixed text)."""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    found = re.findall(r"\b(int|size_t|void|const char\s*\*)\s*(rs_[a-z0-9_]+)\s*\(\s*(const\s+)?rs_ctx\s*\*\s*ctx\b", src)
    names = [n for _, n, _ in found]
    assert len(names) == len(set(names)) and len(names) >= 60
    return {n: (t, bool(c)) for t, n, c in found}


def build(tmp, name, extra):
    exe = os.path.join(tmp, name)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-g", "-O1"] + extra + [MAIN, "-o", exe], check=True, capture_output=True, text=True)
    return exe


@pytest.fixture(scope="module", params=["plain", "asan"])
def exe(request, tmp_path_factory):
    extra = [] if request.param == "plain" else ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    return build(str(tmp_path_factory.mktemp("family")), "family_" + request.param, extra)


def run(exe, mode):
    r = subprocess.run([exe, mode], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout, r.stderr)
    return r.stdout.splitlines()


def table(exe):
    rows = {}
    for line in run(exe, "dump"):
        name, serves, final, hint = (line.split(" ", 3) + [""])[:4]
        assert name not in rows, f"two rows for {name}"
        rows[name] = (int(serves), int(final), hint)
    return rows


def test_the_header_includes_no_hip():
    text = open(os.path.join(CSRC, "rs_family.h")).read()
    assert "hip" not in re.sub(r"//.*", "", text).lower()
    main = open(MAIN).read()
    assert re.findall(r'#include "([^"]+)"', main) == ["../reazonspeech_amd/csrc/rs_family.h"]


def test_one_row_per_context_taking_function(exe):
    rows = table(exe)
    assert sorted(rows) == sorted(declared_entries())
    for name, (serves, final, hint) in rows.items():
        assert 1 <= serves <= 7 and final in (0, 1), name
        assert serves == 7 or hint, f"{name} refuses a family without saying where that family goes"


def test_family_names(exe):
    assert dict((int(k), v) for k, v in (line.split(" ", 1) for line in run(exe, "names"))) == FAMILIES


def test_guard_order_and_codes_for_every_combination(exe):
    rows = table(exe)
    returns = declared_entries()
    seen = set()
    for line in run(exe, "guard"):
        name, have, fam, fin, rc, msg = (line.split(" ", 5) + [""])[:6]
        have, fam, fin, rc = int(have), int(fam), int(fin), int(rc)
        serves, final, hint = rows[name]
        seen.add((name, have, fam, fin))
        if not have:
            want = RS_EINVAL
        elif not serves & (1 << fam):
            want = RS_EINVAL                              # before the finalized test: refused without any weights
        elif final and not fin:
            want = RS_ESTATE
        else:
            want = RS_OK
        assert rc == want, line
        if rc == RS_OK:
            assert msg == "", line
            continue
        assert msg and name in msg, line                  # (every refusal; the int-returning entries hand it to rs_last_error)
        if have and rc == RS_EINVAL:
            assert f"{name}: not defined for {FAMILIES[fam]} context" in msg and hint in msg, line
        if rc == RS_ESTATE:
            assert msg == f"rs_finalize must precede {name}", line
    assert len(seen) == len(rows) * 12
    assert {t for t, _ in returns.values()} >= {"int", "size_t"} and not returns["rs_encoder_forward"][1] and returns["rs_mel_frames"] == ("int", True)


def test_texts_that_callers_and_tests_rely_on(exe):
    rows = table(exe)
    for name in ("rs_rnnt_mbs", "rs_rnnt_mbs_hotwords"):                     # tests/test_gpu_k2_mbs.py, test_gpu_k2_hotwords.py: match="Zipformer"
        assert rows[name][0] == 2 and "Zipformer" in rows[name][2]
    for name in ("rs_rnnt_alsd", "rs_rnnt_beam"):
        assert rows[name][0] == 1 and "stateless decoder; only rs_rnnt_greedy applies" in rows[name][2]
    assert "rs_k2_encoder_set_taps" in rows["rs_encoder_set_taps"][2]
    # tests/test_gpu_token_scores.py pins RS_EINVAL for a context that is not finalized: the entry tests that itself
    assert rows["rs_rnnt_token_scores"][:2] == (3, 0) and rows["rs_rnnt_token_scores_workspace_bytes"][:2] == (3, 1)
    assert all(rows[n][0] == 7 for n in ("rs_gemm_bf16", "rs_gemm_f32", "rs_gemm_i8q", "rs_layernorm", "rs_destroy", "rs_last_error", "rs_set_option"))
    assert all(rows[n][0] == 1 for n in ("rs_relpos_attention", "rs_relpos_attention_f32"))
    assert all(rows[n][0] == 4 for n in rows if n.startswith("rs_avsr_"))


# ---- source checks ---------------------------------------------------------------------------------------------------------------

def csrc_text():
    return {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".h"))}


def test_the_guard_is_the_first_statement_of_every_entry():
    text = csrc_text()
    for name, (ret, query) in declared_entries().items():
        pat = re.compile(r"^(?:extern \"C\" )?" + re.escape(ret).replace(r"\ ", r"\s*") + r"\s*" + name + r"\((?:const )?rs_ctx\* ctx[^{;]*\{\n\s*(.*)\n", flags=re.M)
        hits = [m.group(1) for t in text.values() for m in pat.finditer(t)]
        assert len(hits) == 1, (name, hits)
        query = query or ret == "void"                    # rs_destroy: nothing to return, nowhere to leave a text
        assert hits[0].startswith(f"RS_GUARD_QUERY(ctx, {name}," if query else f"RS_GUARD(ctx, {name})"), (name, hits[0])


def test_nothing_but_the_accessors_asks_for_a_family_state():
    for f, t in csrc_text().items():
        assert not re.search(r"ctx->(k2|avsr)\b", t), f
        if f != "rs_common.h":
            assert "ctx->state" not in t.replace("ctx->state.reset(", "").replace("static_cast<rs_k2*>(ctx->state.get())", "").replace(
                "static_cast<rs_avsr*>(ctx->state.get())", ""), f
    body = text_of_struct(csrc_text()["rs_common.h"], "rs_ctx")
    for field in ("head_dim", "sub_freq", "sub_conv0_w", "sub_dw_w", "sub_pw_w", "sub_out_w", "layers", "fe_mvn_mean", "final_norm_g", "ctc_w", "ctc_probs",
                  "rs_f32_weights", "tap_sub", "tap_layers", "tap_ids", "fuse_glu", "defer_out_norm", "k2_free", "avsr_free"):
        assert not re.search(r"\b" + field + r"\b", body), field


def text_of_struct(text, name):
    start = text.index("struct " + name + " {")
    return text[start:text.index("\n};", start)]


def test_no_throwing_lookup_of_a_registered_tensor():
    for f, t in csrc_text().items():
        assert ".at(" not in t, f
