"""CPU: the table of A/B switches (reazonspeech_amd/csrc/rs_knobs.h).

A stand-alone program (tests/knobs_host_main.cpp) is built from the header with g++ under AddressSanitizer + UBSan and once more
under ThreadSanitizer, and run as a child process per case: the table reads the environment once per process, so every case needs
a fresh one.  The source checks below keep the table the only reader of the environment in csrc/ and every switch that a script or
test names a row of it."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "reazonspeech_amd", "csrc")
HEADER = os.path.join(CSRC, "rs_knobs.h")
MAIN = os.path.join(ROOT, "tests", "knobs_host_main.cpp")
RS_EINVAL = -1

# variables of the Python side (reazonspeech_amd/**/*.py, bench.py and the scripts themselves read them with os.environ): not switches
# of the library.  RS_DECODE_SCREEN / RS_DECODE_NARROW are read on both sides and are rows as well.
PYTHON_SIDE = {"RS_BUFFER_SETS", "RS_DEC_STREAMS", "RS_ENC_STREAMS", "RS_DECODE_PRIORITY", "RS_DECODE_CUS", "RS_NUMA_BIND",
               "RS_DECODE_SCREEN", "RS_DECODE_NARROW"}


def table():
    """[(identifier, environment name, kind, default)] parsed from the X-macro lines"""
    rows = re.findall(r'^\s*X\((\w+),\s*"(RS_\w+)",\s*(PRESENT|INT),\s*(-?\d+),\s*"[^"]*"\)', open(HEADER).read(), flags=re.M)
    assert len(rows) >= 26
    return [(i, e, k, int(d)) for i, e, k, d in rows]


def build(tmp, name, sanitize):
    exe = os.path.join(tmp, name)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-g", "-O1", "-pthread", "-fsanitize=" + sanitize, "-fno-sanitize-recover=all",
                    MAIN, "-o", exe], check=True, capture_output=True, text=True)
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build(str(tmp_path_factory.mktemp("knobs")), "knobs_asan", "address,undefined")


def run(exe, mode, **env):
    base = {k: v for k, v in os.environ.items() if not k.startswith("RS_")}
    base.update(env)
    r = subprocess.run([exe, mode], env=base, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout, r.stderr)
    return r.stdout


def dump(exe, **env):
    out = {}
    for line in run(exe, "dump", **env).splitlines():
        name, value, given = line.split()
        out[name] = (int(value), bool(int(given)))
    return out


def test_nothing_set_gives_the_declared_defaults(exe):
    got = dump(exe)
    assert got == {env: (default, False) for _, env, _, default in table()}
    assert (got["RS_ATTN64"], got["RS_ATTN64_NW"], got["RS_GEMM_PAIRS"], got["RS_BEAM_SPEC"]) == ((4, False), (4, False), (2, False), (3, False))


def test_present_kind_counts_any_text_as_set(exe):
    present = [env for _, env, kind, _ in table() if kind == "PRESENT"]
    assert "RS_ATTN_F32_OLD" in present and "RS_SUB_IM2COL" in present
    got = dump(exe, **{env: "0" for env in present})
    for env in present:
        assert got[env] == (1, True), env
    assert got["RS_GEMM_TILE"] == (0, False)


def test_int_kind_is_atoi_of_the_text(exe):
    ints = [env for _, env, kind, _ in table() if kind == "INT" and env != "RS_ATTN64_NW"]
    got = dump(exe, **{env: "3" for env in ints})
    for env in ints:
        assert got[env] == (3, True), env
    assert dump(exe, RS_K2_CONV2_FUSED="0", RS_GEMM_TILE="192")["RS_K2_CONV2_FUSED"] == (0, True)


def test_attn64_fills_two_rows_from_one_variable(exe):
    got = dump(exe, RS_ATTN64="2,3")
    assert (got["RS_ATTN64"], got["RS_ATTN64_NW"]) == ((2, True), (3, True))
    got = dump(exe, RS_ATTN64="0")
    assert (got["RS_ATTN64"], got["RS_ATTN64_NW"]) == ((0, True), (4, True))       # a missing second number means 4
    got = dump(exe, RS_ATTN64_NW="2")                                               # the second row is not a variable of its own
    assert (got["RS_ATTN64"], got["RS_ATTN64_NW"]) == ((4, False), (4, False))


def test_set_then_get_and_the_environment_is_read_once(exe):
    out = dict(line.split(" ", 1) for line in run(exe, "setget", RS_GEMM_TILE="256").splitlines())
    assert out["first"] == "256"
    assert out["after_setenv"] == "256 0 4 4"         # setenv after the first read changes nothing
    assert out["set_rc"] == "0 0"
    assert out["after_set"] == "128 128 3"
    assert out["given"] == "1"
    out = dict(line.split(" ", 1) for line in run(exe, "setget").splitlines())
    assert (out["first"], out["after_setenv"], out["after_set"], out["given"]) == ("0", "0 0 4 4", "128 128 3", "0")


def test_unknown_name_is_einval(exe):
    assert run(exe, "unknown").split() == [str(RS_EINVAL), str(RS_EINVAL), "7", str(RS_EINVAL), str(RS_EINVAL)]


def test_readers_and_a_writer_under_thread_sanitizer(tmp_path):
    tsan = build(str(tmp_path), "knobs_tsan", "thread")
    assert run(tsan, "threads", RS_GEMM_PAIRS="1").strip() == "done 1"


# ---- source checks ---------------------------------------------------------------------------------------------------------------

def csrc_files():
    return sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".h", ".cpp")))


def test_only_the_table_reads_the_environment():
    for f in csrc_files():
        if f != "rs_knobs.h":
            assert "getenv" not in open(os.path.join(CSRC, f)).read(), f
    assert open(HEADER).read().count("getenv(") == 1


def test_every_row_is_read_somewhere():
    text = "".join(open(os.path.join(CSRC, f)).read() for f in csrc_files() if f != "rs_knobs.h")
    read = set(re.findall(r"\brs_knob\(RS_KNOB_(\w+)\)", text))
    assert read == {ident for ident, _, _, _ in table()}


def names_set_by(path):
    """the RS_* names a script or test sets: os.environ[..] = / .setdefault / .pop, monkeypatch.setenv / delenv, a shell NAME=value
    word (prefix of a command, `env NAME=value`, a list of such words in a for loop), or a name passed to the setter / the helper"""
    text = open(path, encoding="utf-8").read()
    names = set()
    if path.endswith(".py"):
        names |= set(re.findall(r"""os\.environ(?:\[|\.(?:setdefault|pop)\()\s*["'](RS_[A-Z0-9_]+)["']""", text))
        names |= set(re.findall(r"""monkeypatch\.(?:setenv|delenv)\(\s*["'](RS_[A-Z0-9_]+)["']""", text))
        names |= set(re.findall(r"""(?:rs_debug_[sg]et_knob|\bknob|[sg]et_knob)\([^()"']*b?["'](RS_[A-Z0-9_]+)["']""", text))
        for line in text.splitlines():                      # a usage line in a docstring: NAME=value python scripts/...
            if "python " in line:
                names |= set(re.findall(r"\b(RS_[A-Z0-9_]+)=", line))
    else:
        text = "\n".join(line for line in text.splitlines() if not line.lstrip().startswith("#"))
        names |= set(re.findall(r"\b(RS_[A-Z0-9_]+)=", text))
    return names


def test_scripts_and_tests_name_only_switches_that_exist():
    known = {env for _, env, _, _ in table()} | PYTHON_SIDE
    seen = set()
    for sub in ("scripts", "tests"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, sub)):
            for f in files:
                if f.endswith((".py", ".sh")) and f != os.path.basename(__file__):
                    found = names_set_by(os.path.join(dirpath, f))
                    assert found <= known, (f, sorted(found - known))
                    seen |= found
    # the scan sees what it is meant to see
    assert {"RS_ATTN64", "RS_SUB_IM2COL", "RS_BEAM_SPEC", "RS_K2_ATTW_SWEEPS", "RS_GEMM_BREG", "RS_DECODE_NO_LOOKAHEAD"} <= seen
