"""CPU: reading and flattening n-gram language models (reazonspeech_amd/runtime/ngram_lm.py) and the host validator of the flat table
(reazonspeech_amd/csrc/rs_ngram_check.h, exported as rs_ngram_check).  What needs no GPU:

  * the hand-written fixture tests/golden/toy_3gram.arpa: what is read, what is dropped (one warning), the arrays
  * `step` over the flat arrays (include/rs_asr.h) against a textbook dictionary implementation of ARPA backoff in float64, for every
    (history <= 4 tokens, token) of a small vocabulary, in all three token encodings; the bound is derived from float32 rounding
  * the cases: a missing suffix n-gram, a context with no extensions, a file with no `<s>`, a file with no `<unk>`
  * every refusal of the reader
  * rs_ngram_check on each kind of corrupt table, through the library and through a stand-alone program built from the header alone
    with g++ -Wall -Werror, once plain and once under AddressSanitizer + UBSan"""
import itertools
import os
import re
import subprocess
import warnings

import numpy as np
import pytest

import ngram_lm_ref as NR
from reazonspeech_amd.runtime import capi, ngram_lm as NL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "tests", "ngram_host_main.cpp")
BOS = NL.BOS
V, BLANK = 8, 8


def read(path, mode="ids", pieces=None, vocab=V, blank=BLANK):
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        g = NL.read_arpa(path, vocab, blank, mode, pieces)
    return g, [str(x.message) for x in w]


# ---- the fixture -------------------------------------------------------------------------------------------------------------------
def test_fixture_is_read_as_written():
    text = open(NR.TOY_ARPA).read()
    assert len(text.splitlines()) < 60
    for v in re.findall(r"(?m)^(-?[0-9.]+)\t|\t(-?[0-9.]+)$", text):
        x = float(v[0] or v[1])
        assert x * 8 == int(x * 8), x                          # every value a multiple of 1/8
    g, warned = read(NR.TOY_ARPA)
    assert len(warned) == 1 and "3 (</s>)" in warned[0] and "2 (no token id)" in warned[0]
    assert g.order == 3 and g.unk == -1.5 and g.dropped == {"</s>": 3, "<s> not first": 0, "no token id": 2, "blank": 0}
    assert len(g.entries) == 7 + 7 + 4 and g.entries[(BOS, 0, 1)] == (-0.125, 0.0) and g.entries[(5,)] == (-1.75, 0.0)
    lm = NL.build(g, V, BLANK)
    a = lm.arrays
    assert (lm.n_nodes, lm.n_children, lm.n_logits, lm.order) == (19, 17, 9, 3)
    assert lm.start == 1 and a["level"][lm.start] == 1 and lm.start not in a["child_node"]           # `<s>`: no token reaches it
    assert a["root_child"].tolist() == [2, 3, 4, 5, 6, 7, -1, -1, -1]
    assert lm.unk_logp == np.float32(-1.5 * np.log(10.0))
    assert all(a["logp"][n] == np.float32(float(p) * np.log(10.0)) for n, p in [(2, -0.75), (8, -0.25), (15, -0.125)])
    assert a["backoff"][7] == 0.0                              # "5" has no backoff in the file
    n123 = NR.walk(lm, [1, 2], state=0)
    assert a["level"][n123] == 2
    lp, nxt, nb = NR.step(lm, n123, 3)                         # (1 2 3) is there, its suffix (2 3) is not: the longest present is (3)
    assert nb == 0 and nxt == a["root_child"][3] and lp == np.float32(-0.375 * np.log(10.0))
    capi.ngram_check(a, lm.start, lm.order, lm.unk_logp)
    assert NL.build(g, V, BLANK).key == lm.key and NL.build(read(NR.TOY_ARPA)[0], V + 1, V + 1).key != lm.key


def test_fixture_gz_and_blank(tmp_path):
    import gzip
    gz = tmp_path / "toy.arpa.gz"
    with gzip.open(gz, "wb") as fh:
        fh.write(open(NR.TOY_ARPA, "rb").read())
    assert read(str(gz))[0].entries == read(NR.TOY_ARPA)[0].entries
    g, warned = read(NR.TOY_ARPA, vocab=6, blank=3)             # token 3 is the blank of this model: its n-grams go
    assert g.dropped["blank"] == 3 and (3,) not in g.entries and (5, 3) not in g.entries and (1, 2, 3) not in g.entries and len(warned) == 1
    NL.build(g, 6, 3)


# ---- step == textbook backoff ------------------------------------------------------------------------------------------------------
def _random_entries(rng, order, vocab, bos=True, density=1.2):
    ent = {(t,): (-float(rng.integers(4, 40)) / 8.0, -float(rng.integers(0, 12)) / 8.0) for t in range(vocab)
           if (rng.random() < 0.8 or t == 0) and t != vocab - 1}        # the last token never has a unigram: an unknown word
    if bos:
        ent[(BOS,)] = (-99.0, -0.375)
    for n in range(2, order + 1):
        ctxs = [k for k in ent if len(k) == n - 1]
        for k in ctxs:
            for t in range(vocab):
                if (t,) in ent and rng.random() < density / n:
                    ent[k + (t,)] = (-float(rng.integers(1, 30)) / 8.0 - 1.0 / 3.0, -float(rng.integers(0, 9)) / 7.0 if n < order else 0.0)
        if not any(len(k) == n for k in ent):                   # every order of the model has an n-gram
            ent[ctxs[-1] + (0,)] = (-0.625, -0.25 if n < order else 0.0)
    return ent


def _compare(lm, arpa, vocab, has_bos, max_hist=4):
    """every (history <= max_hist tokens, token): step over the flat arrays == the dictionary, within the float32 rounding bound"""
    a = lm.arrays
    M = max(float(np.abs(a["logp"][[n for n in range(lm.n_nodes) if not (has_bos and n == lm.start)]]).max()), float(np.abs(a["backoff"]).max()),
            abs(float(lm.unk_logp)))
    # lp is a sum of at most order backoffs and one log-probability: k = order + 1 stored values, each the float32 rounding of a float64
    # product (relative error 2^-24), added by at most k float32 additions, each rounding a partial sum of magnitude <= k M (relative
    # error 2^-24): |error| <= k M 2^-24 + k (k M) 2^-24 = k (k + 1) M 2^-24
    k = lm.order + 1
    bound = k * (k + 1) * M * 2.0 ** -24
    worst, n = 0.0, 0
    starts = [((), 0)] + ([((BOS,), lm.start)] if has_bos else [])
    for prefix, s0 in starts:
        for hl in range(max_hist + 1):
            for hist in itertools.product(range(vocab), repeat=hl):
                s = NR.walk(lm, hist, state=s0)
                for t in range(vocab):
                    lp, nxt, _ = NR.step(lm, s, t)
                    want = arpa.logp(prefix + hist, t)
                    worst = max(worst, abs(float(lp) - want))
                    assert abs(float(lp) - want) <= bound, (prefix, hist, t, float(lp), want, bound)
                    assert 0 <= nxt < lm.n_nodes and a["level"][nxt] < lm.order
                    n += 1
    return worst, bound, n


@pytest.mark.parametrize("mode,order,bos,unk", [("ids", 3, True, True), ("nemo", 4, True, False), ("pieces", 2, False, True),
                                                ("nemo", 1, False, False), ("ids", 4, False, True)])
def test_step_matches_textbook_backoff(tmp_path, mode, order, bos, unk):
    rng = np.random.default_rng(order * 10 + bos)
    vocab = 5
    pieces = ["▁a", "b", "▁cd", "e", "▁", "x"]
    ent = _random_entries(rng, order, vocab, bos)
    words = dict(ent)
    if unk:
        words[("<unk>",)] = (-2.625, None)
    words[("</s>",)] = (-1.0, None)
    path = NR.write_arpa(str(tmp_path / "lm.arpa"), words, mode, pieces)
    g, warned = read(path, mode, pieces, vocab=vocab, blank=vocab)
    assert g.entries == ent and g.order == order and len(warned) == 1 and "1 (</s>)" in warned[0]
    lm = NL.build(g, vocab, vocab)
    capi.ngram_check(lm.arrays, lm.start, lm.order, lm.unk_logp)
    assert (lm.start != 0) == bos
    floor = min(p for k, (p, _) in list(ent.items()) + [(("</s>",), (-1.0, None))] if len(k) == 1 and k != (BOS,))
    unk10 = -2.625 if unk else floor                            # no `<unk>`: the lowest unigram log-probability of the file
    assert lm.unk_logp == np.float32(unk10 * np.log(10.0))
    worst, bound, n = _compare(lm, NR.ArpaDict(ent, order, unk10), vocab, bos)
    print(f"{mode} order {order}: {n} (history, token) pairs, worst |step - textbook| = {worst:.3g}, bound {bound:.3g}")
    assert (vocab - 1,) not in ent


def test_named_cases(tmp_path):
    """a missing suffix n-gram, a context with no extensions, no `<s>`, no `<unk>`: the dictionary and the arrays agree on each"""
    ent = {(0,): (-1.0, -0.5), (1,): (-1.25, -0.25), (2,): (-0.75, -0.125), (3,): (-2.0, 0.0),
           (0, 1): (-0.5, -0.375), (1, 2): (-0.25, -0.75), (2, 3): (-0.375, -0.625),
           (0, 1, 2): (-0.125, 0.0)}                            # (0 1 2) without ... (1 2) is there; (2 3) is a context with no extensions
    ent_missing = dict(ent)
    del ent_missing[(1, 2)]                                     # now (0 1 2) has no suffix bigram: the longest present suffix is (2)
    for e in (ent, ent_missing):
        path = NR.write_arpa(str(tmp_path / "c.arpa"), e, "ids")
        g, warned = read(path, vocab=5, blank=5)
        assert not warned and g.unk is None and g.floor == -2.0
        lm = NL.build(g, 5, 5)
        assert lm.start == 0 and lm.unk_logp == np.float32(-2.0 * np.log(10.0))
        capi.ngram_check(lm.arrays, lm.start, lm.order, lm.unk_logp)
        _compare(lm, NR.ArpaDict(e, 3, -2.0), 5, False)
        s = NR.walk(lm, [0, 1], state=0)
        lp, nxt, nb = NR.step(lm, s, 2)
        assert nb == 0 and lp == np.float32(-0.125 * np.log(10.0))
        want = (1, 2) if (1, 2) in e else (2,)
        assert lm.arrays["level"][nxt] == len(want)             # full order: popped to the longest suffix the file has
        s23 = NR.walk(lm, [2, 3], state=0)
        assert lm.arrays["level"][s23] == 2 and lm.arrays["child_begin"][s23] == lm.arrays["child_begin"][s23 + 1]
        lp, nxt, nb = NR.step(lm, s23, 0)                       # (2 3) has no extension: its backoff, then (3)'s, then the unigram
        assert nb == 2 and abs(float(lp) - (-0.625 + 0.0 - 1.0) * np.log(10.0)) < 1e-5
        lp, nxt, nb = NR.step(lm, 0, 4)                         # token 4 has no unigram
        assert nxt == 0 and lp == lm.unk_logp


def test_nemo_words_that_python_takes_for_whitespace(tmp_path):
    """chr(id + 100) for id 33 is U+0085 and for id 60 U+00A0: str.split() and str.strip() would eat them"""
    ent = {(33,): (-1.0, -0.5), (60,): (-1.5, -0.25), (33, 60): (-0.25, 0.0), (60, 33): (-0.5, 0.0)}
    path = NR.write_arpa(str(tmp_path / "ws.arpa"), ent, "nemo")
    g, warned = read(path, "nemo", vocab=64, blank=64)
    assert g.entries == {k: (p, b) for k, (p, b) in ent.items()} and not warned


# ---- refusals of the reader ----------------------------------------------------------------------------------------------------------
GOOD = {(0,): (-1.0, -0.5), (1,): (-1.25, None), (0, 1): (-0.5, None)}


def _text(tmp_path, text, name="bad.arpa"):
    p = tmp_path / name
    p.write_text(text, encoding="utf-8")
    return str(p)


def test_reader_refusals(tmp_path):
    good = open(NR.write_arpa(str(tmp_path / "good.arpa"), GOOD, "ids")).read()
    assert read(str(tmp_path / "good.arpa"))[0].entries == {(0,): (-1.0, -0.5), (1,): (-1.25, 0.0), (0, 1): (-0.5, 0.0)}
    cases = {
        "count": (good.replace("ngram 1=2", "ngram 1=3"), r":\d+: the header gives 3 1-grams, the section has 2"),
        "malformed": (good.replace("-1.25\t1", "-1.25\t1 0"), r":7: malformed 1-gram line"),
        "number": (good.replace("-1.25\t1", "minus\t1"), r":7: log-probability 'minus' is not a number"),
        "nan": (good.replace("-1.0\t0\t-0.5", "-1.0\t0\tnan"), r":6: backoff 'nan' is not finite"),
        "inf": (good.replace("-0.5\t0 1", "-inf\t0 1"), r":\d+: log-probability '-inf' is not finite"),
        "prefix": (good.replace("-0.5\t0 1", "-0.5\t2 1"), r"the prefix of the 2-gram '2 1' is not a 1-gram of the file"),
        "no end": (good.replace("\\end\\\n", ""), r"no \\end\\ line"),
        "no data": (good.replace("\\data\\", "data"), r":1: expected \\data\\"),
        "section": (good.replace("\\2-grams:", "\\3-grams:"), r"section 3-grams out of order"),
        "twice": (good.replace("-1.25\t1", "-1.25\t0"), r"occurs twice"),
    }
    for name, (text, pattern) in cases.items():
        assert text != good, name
        with pytest.raises(ValueError, match=pattern):
            NL.read_arpa(_text(tmp_path, text), V, BLANK, "ids")
    nine = "\\data\\\n" + "".join(f"ngram {n}=1\n" for n in range(1, 10)) + "\n"
    with pytest.raises(ValueError, match=r":10: order 9 is above the 8"):
        NL.read_arpa(_text(tmp_path, nine), V, BLANK, "ids")
    binary = tmp_path / "lm.binary"
    binary.write_bytes(NL.KENLM_MAGIC + b" 5\n\x00" + bytes(64))
    with pytest.raises(ValueError, match="only ARPA text is read"):
        NL.read_arpa(str(binary), V, BLANK)
    with pytest.raises(ValueError, match="ngram_lm_tokens"):
        NL.read_arpa(str(tmp_path / "good.arpa"), V, BLANK, "words")
    with pytest.raises(ValueError, match="piece strings"):
        NL.read_arpa(str(tmp_path / "good.arpa"), V, BLANK, "pieces")
    g, warned = read(_text(tmp_path, good.replace("-0.5\t0 1", "-0.5\t1 <s>")))
    assert g.dropped["<s> not first"] == 1 and len(warned) == 1
    for bad in ({(0, 1): (-1.0, 0.0)}, {(0,): (float("nan"), 0.0)}, {(V,): (-1.0, 0.0)}, {(BLANK,): (-1.0, 0.0)}, {(0,): (-1.0, 0.0), (0, BOS): (-1.0, 0.0)}):
        with pytest.raises(ValueError):
            NL.build(bad, V, BLANK)
    with pytest.raises(ValueError, match="order"):
        NL.build(NL.Ngrams(9, {(0,): (-1.0, 0.0)}), V, BLANK)


# ---- the validator -----------------------------------------------------------------------------------------------------------------
def _toy():
    return NL.build(read(NR.TOY_ARPA)[0], V, BLANK)


def _corruptions():
    """name -> (what to change in a copy of the toy table, the reason rs_ngram_check gives)"""
    def edit(key, idx, val):
        def f(a, s):
            a[key][idx] = val
        return f

    def scalar(name, val):
        def f(a, s):
            s[name] = val
        return f
    return {
        "order 0": (scalar("order", 0), "order 0 outside 1..8"),
        "order 9": (scalar("order", 9), "order 9 outside 1..8"),
        "start deep": (scalar("start", 8), "start=8 is neither the root nor a level-1 node"),
        "start outside": (scalar("start", 19), "start=19 is neither"),
        "unk nan": (scalar("unk_logp", float("nan")), "unk_logp is not finite"),
        "child_begin end": (edit("child_begin", 19, 16), "child_begin must run from 0 to n_children=17"),
        "child_begin descending": (edit("child_begin", 3, 7), "not an ascending range"),
        "child outside": (edit("child_node", 6, 19), "child_node[6]=19 outside the nodes"),
        "child is root": (edit("child_node", 6, 0), "child_node[6]=0 outside the nodes"),
        "child level": (edit("child_node", 6, 15), "child 15 of node 1 is not one level below it"),
        "children unsorted": (edit("child_tok", 1, 0), "children of node 0 are not sorted ascending"),
        "token outside": (edit("child_tok", 16, 9), "child_tok[16]=9 outside the 9 logits"),
        "suffix outside": (edit("suffix", 9, -1), "suffix[9]=-1 outside"),
        "suffix level": (edit("suffix", 9, 10), "suffix[9]=10 does not lower the level"),
        "root suffix": (edit("suffix", 0, 2), "the root (node 0) must have level 0 and itself as suffix"),
        "level above order": (scalar("order", 2), "level[15]=3 outside 0..order=2"),
        "root_child wrong node": (edit("root_child", 0, 3), "root_child[0]=3 is not the root's child on that token"),
        "root_child deep": (edit("root_child", 6, 8), "root_child[6]=8 is not a level-1 node"),
        "root_child missing": (edit("root_child", 2, -1), "the root has 6 children but root_child lists 5"),
        "root_child start": (edit("root_child", 7, 1), "root_child[7]=1 is not the root's child"),
        "logp inf": (edit("logp", 5, float("-inf")), "node 5 has a value that is not finite"),
        "backoff nan": (edit("backoff", 12, float("nan")), "node 12 has a value that is not finite"),
    }


def _apply(change):
    lm = _toy()
    a = {k: v.copy() for k, v in lm.arrays.items()}
    s = dict(start=lm.start, order=lm.order, unk_logp=float(lm.unk_logp))
    change(a, s)
    return a, s


def test_ngram_check_through_the_library():
    lm = _toy()
    capi.ngram_check(lm.arrays, lm.start, lm.order, lm.unk_logp)
    for name, (change, reason) in _corruptions().items():
        a, s = _apply(change)
        with pytest.raises(capi.RsError, match=re.escape(reason)) as e:
            capi.ngram_check(a, s["start"], s["order"], s["unk_logp"])
        assert e.value.code == capi.RS_EINVAL, name
    short = {k: v.copy() for k, v in lm.arrays.items()}
    short["suffix"] = short["suffix"][:-1]
    with pytest.raises(capi.RsError, match="disagree in length"):
        capi.ngram_check(short, lm.start, lm.order, lm.unk_logp)
    lib = capi.load()
    assert lib.rs_ngram_check(None, None, 0) == capi.RS_EINVAL
    empty = capi.RsNgram()                                       # n_nodes == 0: no model, nothing to refuse
    assert lib.rs_ngram_check(empty, None, 0) == capi.RS_OK


def _block(a, s):
    n = lambda v: "nan" if v != v else ("inf" if v == float("inf") else "-inf" if v == float("-inf") else repr(float(v)))   # noqa: E731
    head = f"{len(a['logp'])} {len(a['child_tok'])} {len(a['root_child'])} {s['order']} {s['start']} {n(s['unk_logp'])}"
    rows = [f"{len(a[k])} " + " ".join(n(v) if k in NL.FLOATS else str(int(v)) for v in a[k]) for k in NL.ARRAYS]
    return "\n".join([head] + rows) + "\n"


@pytest.fixture(scope="module", params=["plain", "asan"])
def exe(request, tmp_path_factory):
    extra = [] if request.param == "plain" else ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    out = os.path.join(str(tmp_path_factory.mktemp("ngram")), "ngram_" + request.param)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-g", "-O1"] + extra + [MAIN, "-o", out], check=True, capture_output=True, text=True)
    return out


def test_the_header_is_hip_free_and_stands_alone():
    text = open(os.path.join(ROOT, "reazonspeech_amd", "csrc", "rs_ngram_check.h")).read()
    assert "hip" not in re.sub(r"//.*", "", text).lower()
    assert re.findall(r'#include "([^"]+)"', open(MAIN).read()) == ["../reazonspeech_amd/csrc/rs_ngram_check.h"]
    assert '#include "rs_ngram_check.h"' in open(os.path.join(ROOT, "reazonspeech_amd", "csrc", "rs_api.hip")).read()
    walk = open(os.path.join(ROOT, "reazonspeech_amd", "csrc", "k_rnnt_ngram.h")).read()
    assert re.findall(r'#include "([^"]+)"', walk) == ["k_rnnt_common.h"]        # the walk only: nothing of a search


def test_ngram_check_stand_alone(exe, tmp_path):
    lm = _toy()
    cases = list(_corruptions().items())
    text = _block(lm.arrays, dict(start=lm.start, order=lm.order, unk_logp=float(lm.unk_logp)))
    for _, (change, _) in cases:
        text += _block(*_apply(change))
    big = NL.build(NR.random_lm(type("C", (), {"vocab_size": 300})(), [list(range(0, 300, 7))], n_high=800), 300, 300)
    text += _block(big.arrays, dict(start=big.start, order=big.order, unk_logp=float(big.unk_logp)))
    path = tmp_path / "tables.txt"
    path.write_text(text)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout[-400:], r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases) + 2
    assert lines[0].strip() == "0" and lines[-1].strip() == "0"
    for line, (name, (_, reason)) in zip(lines[1:-1], cases):
        assert line.startswith("-1 ngram: ") and reason in line, (name, line)
