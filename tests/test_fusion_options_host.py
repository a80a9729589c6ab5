"""CPU: the hotword and n-gram LM options of the three packages (nemo: ALSD, k2: modified beam search, espnet: default beam search),
seen from the entry points a caller has — `load_model`, `transcribe` / `transcribe_batch`, `K2Model.create_stream` / `decode_streams`,
`EspnetModel.__call__` / `recognize_batch`, `AsrModel.lm_plan` / `graph_plan` — with the runtime replaced by a recorder where a call
would reach the device.  What is pinned is what the packages do NOT share, so that host code common to them cannot level it out:

  * the full text with which every family refuses an LM and hotwords for every decoding that cannot fuse them, at load time and at
    plan time (the plan speaks the nemo package's words for an espnet model, and lets all three fused searches pass whatever the family)
  * which error a doubly-wrong call gets (the order of the checks in each loader)
  * `hotwords=` of a call over n items: None, the empty string (nemo and k2: the model's graph; espnet: no graph INSTEAD OF the
    model's), one string for all, a list, a list of the wrong length, and what is built once (equal strings everywhere; the same
    object only in espnet)
  * `ngram_lm_alpha=` of a call: None (nemo resolves the model's pair, k2 and espnet leave it to the runtime), 0, a value without an
    LM, and a negative, NaN or bool value."""
import importlib
import types

import numpy as np
import pytest

import espnet_fake
from reazonspeech_amd.espnet.asr import load_model as espnet_load
from reazonspeech_amd.espnet.asr.interface import AudioData as EspnetAudio
from reazonspeech_amd.espnet.asr.model import EspnetModel, synthetic_token_list
from reazonspeech_amd.k2.asr import huggingface as hfm
from reazonspeech_amd.k2.asr.interface import AudioData as K2Audio
from reazonspeech_amd.k2.asr.model import K2Model, search_config, synthetic_tokens
from reazonspeech_amd.nemo.asr import load_model as nemo_load
from reazonspeech_amd.nemo.asr.interface import AudioData as NemoAudio
from reazonspeech_amd.runtime import k2_hotwords as kh, ngram_lm as NL
from reazonspeech_amd.runtime.config import ESPNET_TINY, TINY
from reazonspeech_amd.runtime.k2_config import ZIPFORMER_TINY
from reazonspeech_amd.runtime.model import AsrModel, DecodedBatch
from reazonspeech_amd.runtime.tokenizer import SyntheticTokenizer

nemo_tr = importlib.import_module("reazonspeech_amd.nemo.asr.transcribe")        # (the packages export functions of the same name)
k2_tr = importlib.import_module("reazonspeech_amd.k2.asr.transcribe")
espnet_tr = importlib.import_module("reazonspeech_amd.espnet.asr.transcribe")

FAMILIES = ("nemo", "k2", "espnet")
MBS = "modified_beam_search"
WAVE = np.zeros(160, np.float32)
IDS = (10, 11)                                 # a phrase as token ids: inside every toy vocabulary, neither blank nor <unk>
KEY = ((IDS, 1.5),)                            # ... and the key of its graph at the default score

# the refusals, copied from the packages: "{}" is the decoding's repr
NEMO_LM = "an n-gram LM needs decoding='alsd', not {}"
NEMO_HW = "hotwords need decoding='alsd', not {}"
K2_LM = "an n-gram LM needs decoding_method='modified_beam_search', not {}"
K2_HW_PLAN = "hotwords need decoding_method='modified_beam_search'"
K2_HW = K2_HW_PLAN + " (greedy_search has no hypotheses to bias)"
ESPNET_LM = "an n-gram LM needs the beam search (beam_size > 1): greedy_search has no hypotheses to re-rank"
ESPNET_HW = "hotwords need the beam search (beam_size > 1): greedy_search has no hypotheses to bias"
NO_LM = "ngram_lm_alpha given, but the model has no n-gram LM (load_model(ngram_lm_model=...))"
BAD_ALPHA = "ngram_lm_alpha must be a finite number >= 0, not {}"
PER_AUDIO = ("hotwords: {} entries for {} audios (a list is one entry per audio; pass a string of phrases separated by '/' to use one "
             "specification for all)")
PER_WINDOW = "hotwords: {} entries for {} windows (a list has one entry per window; one spec for all is a string)"
PER_RECORDING = "hotwords: {} entries for {} recordings (a list has one entry per recording; one spec for all is a string)"

CFG = {"nemo": TINY, "k2": ZIPFORMER_TINY, "espnet": ESPNET_TINY}
FUSING = {"nemo": "alsd", "k2": MBS, "espnet": "beam"}
NOT_FUSING = [("nemo", "greedy"), ("nemo", "greedy_batch"), ("nemo", "beam"), ("k2", "greedy_batch"), ("espnet", "greedy"), ("espnet", "greedy_batch")]


def toy_lm(family):
    cfg = CFG[family]
    return NL.build({(10,): (-0.5, 0.0)}, cfg.vocab_size, cfg.blank_id, cfg.n_logits)


def message(call, exc=ValueError):
    with pytest.raises(exc) as e:
        call()
    return str(e.value)


# ---- one model per family whose runtime is a recorder ---------------------------------------------------------------------------
class Nemo:
    """the nemo package: the model is the runtime model itself, `transcribe_batch` / `transcribe` resolve the options"""
    per_item = PER_AUDIO

    def __init__(self, decoding="alsd", own=None, lm=None, alpha=0.0):
        self.cfg, self.tokenizer = TINY.with_(decoding=decoding), SyntheticTokenizer(TINY.vocab_size, 0)
        self.hotwords, self.hotwords_score, self.ngram_lm, self.ngram_lm_alpha = own, 1.5, lm, alpha
        self.device, self.calls = "cpu", []
        self.text = self.tokenizer.pieces[7] + self.tokenizer.pieces[9]

    def transcribe_waveforms(self, waves, on_batch=None, hotwords=None, nbest=None, ngram_lm=None):
        self.calls.append((len(waves), hotwords, ngram_lm))

    def graph(self, spec):
        return self.graphs([spec], 1)[0]

    def graphs(self, hotwords, n):
        nemo_tr.transcribe_batch(self, [NemoAudio(WAVE, 16000)] * n, nemo_tr.TranscribeConfig(verbose=False), hotwords=hotwords)
        return self.calls[-1][1]

    def one(self, hotwords):
        nemo_tr.transcribe(self, NemoAudio(WAVE, 16000), nemo_tr.TranscribeConfig(verbose=False), hotwords=hotwords)
        return self.calls[-1][1]

    def alpha(self, value):
        nemo_tr.transcribe(self, NemoAudio(WAVE, 16000), nemo_tr.TranscribeConfig(verbose=False), ngram_lm_alpha=value)
        return self.calls[-1][2]


class K2:
    """the k2 package: `_streams` builds one stream per audio, `decode_streams` hands their graphs and the weight to the runtime"""
    per_item = PER_AUDIO

    def __init__(self, decoding=MBS, own=None, lm=None, alpha=0.0):
        m = self.model = K2Model.__new__(K2Model)
        m.cfg = ZIPFORMER_TINY.with_(decoding=decoding)
        m.tokens, m.hotwords_score, m.hotwords = synthetic_tokens(m.cfg.vocab_size), 1.5, own
        m.am = types.SimpleNamespace(ngram_lm=lm, ngram_lm_alpha=alpha, nbest=0, token_scores=False, transcribe_waveforms=self.record)
        self.calls = []
        self.text = m.tokens[10] + m.tokens[11]

    def record(self, waves, hotwords=None, ngram_lm=None):
        self.calls.append((len(waves), hotwords, ngram_lm))
        return DecodedBatch([[10]] * len(waves), [[0]] * len(waves), [1] * len(waves), [0.0] * len(waves), [False] * len(waves))

    def graph(self, spec):
        return self.model.hotword_graph(spec)

    def streams(self, hotwords, n):
        return k2_tr._streams(self.model, [K2Audio(WAVE, 16000)] * n, hotwords)

    def graphs(self, hotwords, n):
        self.model.decode_streams(self.streams(hotwords, n))
        return self.calls[-1][1]

    def one(self, hotwords):
        k2_tr.transcribe(self.model, K2Audio(WAVE, 16000), hotwords=hotwords)
        return self.calls[-1][1]

    def alpha(self, value):
        self.model.decode_streams(self.streams(None, 1), ngram_lm_alpha=value)
        return self.calls[-1][2]


class Espnet:
    """the espnet package: `recognize_batch` / `model(speech)` resolve the options for `_search`"""
    per_item = PER_WINDOW

    def __init__(self, decoding="beam", own=None, lm=None, alpha=0.0):
        m = self.model = EspnetModel.__new__(EspnetModel)
        m.cfg = ESPNET_TINY.with_(decoding=decoding, beam_size=4 if decoding == "beam" else 1)
        m.token_list, m.beam_size, m.hotwords = synthetic_token_list(ESPNET_TINY.vocab_size), m.cfg.beam_size, own
        m.am = types.SimpleNamespace(nbest=0, ngram_lm=lm, ngram_lm_alpha=alpha, token_scores=False)
        m._search = self.record
        self.calls = []
        self.text = m.token_list[10] + m.token_list[11]

    def record(self, waves, **kw):
        self.calls.append((len(waves), kw.get("hotwords"), kw.get("ngram_lm")))
        return DecodedBatch([[10]] * len(waves), [[0]] * len(waves), [1] * len(waves), [0.0] * len(waves), [False] * len(waves))

    def graph(self, spec):
        return self.model.hotword_graph(spec)

    def graphs(self, hotwords, n):
        self.model.recognize_batch([WAVE] * n, hotwords=hotwords)
        return self.calls[-1][1]

    def one(self, hotwords):
        self.model(WAVE, hotwords=hotwords)
        return self.calls[-1][1]

    def alpha(self, value):
        self.model(WAVE, ngram_lm_alpha=value)
        return self.calls[-1][2]


MODEL = {"nemo": Nemo, "k2": K2, "espnet": Espnet}


# ---- (a) the refusals -----------------------------------------------------------------------------------------------------------------
def test_nemo_refuses_at_load_time_in_its_words():
    lm = toy_lm("nemo")
    for decoding in ("greedy", "greedy_batch", "beam"):                    # before any device is touched
        load = lambda **kw: nemo_load(device="cuda:0", config=TINY, decoding=decoding, **kw)
        assert message(lambda: load(ngram_lm_model=lm, ngram_lm_alpha=0.3)) == NEMO_LM.format(repr(decoding))
        assert message(lambda: load(ngram_lm_model="lm.arpa")) == NEMO_LM.format(repr(decoding))        # ... and before the file is looked for
        assert message(lambda: load(hotwords=[IDS])) == NEMO_HW.format(repr(decoding))
        assert message(lambda: load(hotwords="x")) == NEMO_HW.format(repr(decoding))
    # the configuration's own strategy is known only after the (synthetic) checkpoint is read: the second pass refuses
    assert message(lambda: nemo_load(device="cuda:0", config=TINY, ngram_lm_model=lm)) == NEMO_LM.format("'greedy_batch'")
    assert message(lambda: nemo_load(device="cuda:0", config=TINY, hotwords=[IDS])) == NEMO_HW.format("'greedy_batch'")


def test_k2_refuses_at_load_time_in_its_words():
    lm = toy_lm("k2")
    calls = (lambda **kw: hfm.load_model(**kw), lambda **kw: search_config(ZIPFORMER_TINY, **kw),
             lambda **kw: K2Model(ZIPFORMER_TINY, {}, synthetic_tokens(ZIPFORMER_TINY.vocab_size), **kw))
    for call in calls:
        for kw in ({}, dict(decoding_method="greedy_search")):
            assert message(lambda: call(ngram_lm_model="lm.arpa", **kw)) == K2_LM.format("'greedy_search'")     # the caller's word
            assert message(lambda: call(ngram_lm_model=lm, ngram_lm_alpha=0.3, **kw)) == K2_LM.format("'greedy_search'")
            assert message(lambda: call(hotwords=[IDS], **kw)) == K2_HW
            assert message(lambda: call(hotwords_file="hot.txt", **kw)) == K2_HW
    greedy = K2("greedy_batch").model
    assert message(lambda: greedy.hotword_graph([IDS])) == K2_HW and message(lambda: greedy.create_stream(hotwords=[IDS])) == K2_HW
    assert greedy.hotword_graph(None) is None and greedy.hotword_graph("") is None and greedy.create_stream().hotwords is None
    assert message(lambda: setattr(greedy, "ngram_lm", lm)) == K2_LM.format("'greedy_batch'")           # the configuration's word
    greedy.ngram_lm = None                                                                                # no model: nothing to refuse
    assert greedy.am.ngram_lm is None


def test_espnet_refuses_at_load_time_in_its_words():
    lm = toy_lm("espnet")
    toks = synthetic_token_list(ESPNET_TINY.vocab_size)
    for call in (lambda **kw: espnet_load(device="cuda:0", config=ESPNET_TINY, **kw), lambda **kw: EspnetModel(ESPNET_TINY, {}, toks, **kw)):
        for kw in ({}, dict(beam_size=1), dict(beam_size=0)):
            assert message(lambda: call(ngram_lm_model=lm, **kw)) == ESPNET_LM
            assert message(lambda: call(ngram_lm_model="lm.arpa", ngram_lm_alpha=0.3, **kw)) == ESPNET_LM
            assert message(lambda: call(hotwords_file="hot.txt", **kw)) == ESPNET_HW
        assert message(lambda: call(ngram_lm_model=lm, hotwords_file="hot.txt")) == ESPNET_LM          # both: the LM's refusal comes first
    for decoding in ("greedy", "greedy_batch"):
        greedy = Espnet(decoding).model
        assert message(lambda: greedy.hotword_graph([IDS])) == ESPNET_HW
        assert message(lambda: greedy.hotword_graph(kh.build_graph([(IDS, 1.5)]))) == ESPNET_HW          # a ready graph is refused too
        assert greedy.hotword_graph(None) is None and greedy.hotword_graph("") is None
        assert message(lambda: setattr(greedy, "ngram_lm", lm)) == ESPNET_LM
        greedy.ngram_lm = None
        assert greedy.am.ngram_lm is None


def plan_model(family, decoding):
    """an AsrModel with nothing but its configuration; the device tables are stood in for by a marker"""
    m = AsrModel.__new__(AsrModel)
    m.cfg = CFG[family].with_(decoding=decoding)
    m.ngram_set = lambda lm: ("lm table", lm)
    m.hotword_set = lambda graphs: ("graph table", graphs)
    return m


@pytest.mark.parametrize("family,decoding", NOT_FUSING)
def test_the_plan_refuses_in_the_words_of_the_transducer_packages(family, decoding):
    m = plan_model(family, decoding)
    lm, g = toy_lm(family), kh.build_graph([(IDS, 1.5)])
    assert m.lm_plan((None, 0.3)) is None and m.lm_plan((lm, 0.0)) is None and m.lm_plan((lm, 0)) is None      # nothing to fuse: no refusal
    assert m.graph_plan(None, 2) is None and m.graph_plan([None, None], 2) is None
    m.ngram_lm, m.ngram_lm_alpha = None, 0.3
    assert m.lm_plan() is None
    m.ngram_lm = lm                                                                                            # the model's own pair
    if decoding == "beam":       # the device fuses in all three searches, and the plan lets each pass whatever the family
        assert m.lm_plan() == (("lm table", lm), 0.3) and m.lm_plan((lm, 2)) == (("lm table", lm), 2.0)
        assert m.graph_plan([None, g], 2) == (("graph table", (g,)), [-1, 0])
        return
    want_lm = K2_LM.format(repr(decoding)) if family == "k2" else NEMO_LM.format(repr(decoding))               # espnet: the nemo package's words
    want_hw = K2_HW_PLAN if family == "k2" else NEMO_HW.format(repr(decoding))
    assert message(lambda: m.lm_plan((lm, 0.3))) == want_lm and message(lambda: m.lm_plan()) == want_lm
    assert message(lambda: m.graph_plan([None, g], 2)) == want_hw
    assert message(lambda: m.graph_plan([g], 2)) == "hotwords: 1 entries for 2 utterances"                     # the count comes first


@pytest.mark.parametrize("family", FAMILIES)
def test_the_plan_of_a_fusing_search(family):
    m = plan_model(family, FUSING[family])
    lm, g, h = toy_lm(family), kh.build_graph([(IDS, 1.5)]), kh.build_graph([((12,), 2.0)])
    assert m.lm_plan((lm, 0.3)) == (("lm table", lm), 0.3) and m.lm_plan((lm, 0.0)) is None and m.lm_plan((None, 0.3)) is None
    for bad in (-0.5, float("nan"), float("inf")):
        assert message(lambda: m.lm_plan((lm, bad))) == BAD_ALPHA.format(repr(bad))
    assert m.graph_plan([g, None, h, g], 4) == (("graph table", (g, h)), [0, -1, 1, 0])
    a_stub = AsrModel.__new__(AsrModel)                                     # a configuration that names no family reads as nemo's
    a_stub.cfg = types.SimpleNamespace(decoding="greedy_batch")
    assert message(lambda: a_stub.lm_plan((lm, 0.3))) == NEMO_LM.format("'greedy_batch'")
    assert message(lambda: a_stub.graph_plan([g], 1)) == NEMO_HW.format("'greedy_batch'")


# ---- which error a doubly-wrong call gets ---------------------------------------------------------------------------------------------
def test_the_order_of_the_checks_in_each_loader(tmp_path):
    nan, missing, lm_missing = float("nan"), str(tmp_path / "missing.txt"), str(tmp_path / "missing.arpa")
    # nemo: the hotwords file, the hotword keywords (only with a decoding given), the LM keywords, the LM file
    load = lambda **kw: nemo_load(device="cuda:0", config=TINY, **kw)
    assert message(lambda: load(decoding="greedy", hotwords_file=missing), FileNotFoundError) == f"hotwords_file {missing!r} does not exist"
    assert message(lambda: load(decoding="alsd", hotwords_file=missing, hotwords_score=nan), FileNotFoundError).startswith("hotwords_file")
    assert message(lambda: load(decoding="alsd", hotwords_score=nan, ngram_lm_alpha=-1)) == "hotwords_score must be a finite number, not nan"
    assert message(lambda: load(decoding="greedy", hotwords_score=nan, hotwords=[IDS])) == "hotwords_score must be a finite number, not nan"
    assert message(lambda: load(decoding="greedy", hotwords=[IDS], ngram_lm_alpha=-1)) == NEMO_HW.format("'greedy'")
    assert message(lambda: load(decoding="alsd", ngram_lm_model=lm_missing, ngram_lm_alpha=-1)) == BAD_ALPHA.format("-1")
    assert message(lambda: load(decoding="alsd", ngram_lm_model=lm_missing, ngram_lm_tokens="words")) == "ngram_lm_tokens must be one of ('nemo', 'pieces', 'ids'), not 'words'"
    assert message(lambda: load(decoding="greedy", ngram_lm_model=lm_missing)) == NEMO_LM.format("'greedy'")
    assert message(lambda: load(decoding="alsd", ngram_lm_model=lm_missing), FileNotFoundError) == f"ngram_lm_model {lm_missing!r} does not exist"
    # ... without a decoding the first hotwords pass is skipped: the LM's file is missed before the score is looked at
    assert message(lambda: load(hotwords_score=nan, ngram_lm_model=lm_missing), FileNotFoundError) == f"ngram_lm_model {lm_missing!r} does not exist"
    assert message(lambda: load(hotwords_score=nan, ngram_lm_alpha=-1)) == BAD_ALPHA.format("-1")
    assert message(lambda: load(hotwords_score=nan)) == "hotwords_score must be a finite number, not nan"       # the second pass
    # k2: nbest, the hotwords score, hotwords with greedy_search, the method's name, the LM keywords, blank_penalty; then the files
    for call in (lambda **kw: search_config(ZIPFORMER_TINY, **kw), lambda **kw: hfm.load_model(**kw)):
        assert message(lambda: call(nbest=9, hotwords=[IDS], hotwords_score=nan)) == "nbest must be an integer in 0..8, not 9"
        assert message(lambda: call(nbest=2, hotwords=[IDS])) == "nbest=2 needs decoding_method='modified_beam_search' (greedy_search keeps one hypothesis)"
        assert message(lambda: call(hotwords=[IDS], hotwords_score=nan)) == "hotwords_score must be a finite number, not nan"
        assert message(lambda: call(hotwords=[IDS], ngram_lm_model="lm.arpa")) == K2_HW
        assert message(lambda: call(decoding_method="beam", hotwords=[IDS], ngram_lm_model="lm.arpa")) == \
            "decoding_method must be 'greedy_search' or 'modified_beam_search', not 'beam'"                      # an unknown method is not "greedy_search"
        assert message(lambda: call(decoding_method=MBS, ngram_lm_alpha=-1, ngram_lm_tokens="nemo", blank_penalty=-1)) == BAD_ALPHA.format("-1")
        assert message(lambda: call(decoding_method=MBS, ngram_lm_tokens="nemo", blank_penalty=-1)) == \
            "ngram_lm_tokens='nemo' is the NeMo package's word encoding; the k2 package reads 'pieces' (the symbols of tokens.txt) or 'ids'"
        assert message(lambda: call(decoding_method=MBS, ngram_lm_tokens="words")) == "ngram_lm_tokens must be one of ('pieces', 'ids'), not 'words'"
        assert message(lambda: call(ngram_lm_model="lm.arpa", blank_penalty=-1)) == K2_LM.format("'greedy_search'")
        assert message(lambda: call(decoding_method=MBS, ngram_lm_model="", blank_penalty=-1)) == "blank_penalty must be >= 0, not -1"
    assert message(lambda: hfm.load_model(decoding_method=MBS, ngram_lm_model=lm_missing, hotwords_file=missing), FileNotFoundError) == \
        f"ngram_lm_model {lm_missing!r} does not exist"
    assert message(lambda: hfm.load_model(decoding_method=MBS, hotwords_file=missing), FileNotFoundError) == f"hotwords_file {missing!r} does not exist"
    assert message(lambda: hfm.load_model(hotwords_file=missing)) == K2_HW                                          # the keywords before the files
    # espnet: alpha, the token encoding, the hotwords score, then the two refusals
    toks = synthetic_token_list(ESPNET_TINY.vocab_size)
    for call in (lambda **kw: espnet_load(device="cuda:0", config=ESPNET_TINY, **kw), lambda **kw: EspnetModel(ESPNET_TINY, {}, toks, **kw)):
        assert message(lambda: call(ngram_lm_model="lm.arpa", ngram_lm_alpha=-1, ngram_lm_tokens="nemo", hotwords_score=nan)) == BAD_ALPHA.format("-1")
        assert message(lambda: call(ngram_lm_model="lm.arpa", ngram_lm_tokens="nemo", hotwords_score=nan)) == \
            "ngram_lm_tokens must be one of ('pieces', 'ids'), not 'nemo' ('pieces' = the symbols of token_list)"
        assert message(lambda: call(ngram_lm_model="lm.arpa", hotwords_score=nan)) == "hotwords_score must be a finite number, not nan"
        assert message(lambda: call(beam_size=4, hotwords_score=True)) == "hotwords_score must be a finite number, not True"
        assert message(lambda: call(nbest=2, ngram_lm_model="lm.arpa")) == "nbest=2 needs the beam search (beam_size > 1): greedy_search keeps one hypothesis"


# ---- (b) `hotwords=` of a call over n items --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
def test_no_hotwords_and_the_models_own(family):
    m = MODEL[family]()
    assert m.graphs(None, 3) is None and m.graphs([None, None, None], 3) is None
    assert m.graphs("", 3) is None and m.graphs(["", None, ""], 3) is None
    own = m.graph([(12,)])
    m = MODEL[family](own=own)
    assert m.graphs(None, 2) == [own, own] and m.graphs([None, None], 2) == [own, own]
    mixed = m.graphs([None, [IDS]], 2)
    assert mixed[0] is own and mixed[1].key == KEY
    # the empty string: the model's graph in nemo and k2; in espnet a string is a spec INSTEAD OF the model's, and an empty one is no graph
    if family == "espnet":
        assert m.graphs("", 2) is None and m.graphs(["", ""], 2) is None
        assert m.graphs(["", None], 2) == [None, own]
    else:
        assert m.graphs("", 2) == [own, own] and m.graphs(["", None], 2) == [own, own]


def test_k2_leaves_the_models_graph_to_decode_time():
    own = kh.build_graph([((12,), 1.5)])
    m = K2(own=own)
    for spec in (None, "", [None, ""]):
        assert [st.hotwords for st in m.streams(spec, 2)] == [None, None]          # the stream has none: `decode_streams` puts the model's in
    st = m.streams([None, [IDS]], 2)
    assert st[0].hotwords is None and st[1].hotwords.key == KEY
    m.model.hotwords = None                                                        # ... the model's graph at DECODE time, not at stream time
    m.model.decode_streams(st)
    assert m.calls[-1][1][0] is None and m.calls[-1][1][1].key == KEY


@pytest.mark.parametrize("family", FAMILIES)
def test_one_spec_for_all_and_what_is_built_once(family):
    m = MODEL[family]()
    all3 = m.graphs(m.text, 3)
    assert len(all3) == 3 and all3[0] is all3[1] is all3[2] and all3[0].n_phrases >= 1
    assert m.graphs(m.text + " :3", 1)[0].key[0][1] == 3.0
    phrases, equal = [IDS], [IDS]
    got = m.graphs([m.text, None, m.text, phrases, phrases, equal], 6)
    assert got[0] is got[2] and got[0].key == all3[0].key and got[1] is None                # equal strings: one graph
    assert got[3].key == got[4].key == got[5].key == KEY and got[5] is not got[3]
    assert (got[3] is got[4]) == (family == "espnet")                                       # the same object twice: shared in espnet only
    ready = kh.build_graph([(IDS, 2.0)])
    assert m.graphs([ready, None], 2) == [ready, None]                                      # a ready graph is taken as it is
    if family == "espnet":
        assert m.graphs(ready, 2) == [ready, ready]                                         # ... in espnet also as the one for every window


@pytest.mark.parametrize("family", FAMILIES)
def test_a_list_of_the_wrong_length_and_a_single_items_list(family):
    m = MODEL[family]()
    assert message(lambda: m.graphs([None, None, None], 2)) == m.per_item.format(3, 2)
    assert message(lambda: m.graphs([], 1)) == m.per_item.format(0, 1)
    assert message(lambda: m.graphs([m.text], 2)) == m.per_item.format(1, 2)
    one = m.one([IDS, (12,)])                                              # transcribe / model(speech): a list is ONE item's phrases
    assert len(one) == 1 and one[0].n_phrases == 2
    assert m.one(None) is None and m.one("") is None and m.one(m.text)[0].n_phrases >= 1
    own = m.graph([(12,)])
    m = MODEL[family](own=own)
    assert m.one(None) == [own] and m.one([IDS])[0].key == KEY
    assert m.one("") == (None if family == "espnet" else [own])


def test_espnet_fans_specs_out_per_recording():
    model = espnet_fake.FakeEspnetModel()
    short = EspnetAudio(espnet_fake.long_audio(1.0, seed=1), 16000)
    assert message(lambda: espnet_tr.transcribe_batch(model, [short] * 3, hotwords=["a", "b"])) == PER_RECORDING.format(2, 3)


@pytest.mark.parametrize("family", FAMILIES)
def test_a_call_with_hotwords_needs_the_fusing_search(family):
    decoding = "greedy_batch"
    m = MODEL[family](decoding)
    want = {"nemo": NEMO_HW.format("'greedy_batch'"), "k2": K2_HW, "espnet": ESPNET_HW}[family]
    assert message(lambda: m.graphs([None, [IDS]], 2)) == want and message(lambda: m.one([IDS])) == want
    assert message(lambda: m.graphs(m.text, 2)) == want
    assert m.graphs(None, 2) is None and m.graphs([None, ""], 2) is None   # nothing asked for: the greedy search is fine


# ---- (c) `ngram_lm_alpha=` of a call ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
def test_the_weight_of_one_call(family):
    lm = toy_lm(family)
    without, has = MODEL[family](), MODEL[family](lm=lm, alpha=0.25)
    # None: nemo resolves the model's own pair, k2 and espnet pass None on ("the runtime's own")
    assert without.alpha(None) == ((None, 0.0) if family == "nemo" else None)
    assert has.alpha(None) == ((lm, 0.25) if family == "nemo" else None)
    assert MODEL[family](lm=lm, alpha=0.0).alpha(None) == ((None, 0.0) if family == "nemo" else None)
    # 0: this call without the LM (espnet hands the table on at weight 0, which the plan reads as no LM)
    assert without.alpha(0) == (None, 0.0) and without.alpha(0.0) == (None, 0.0)
    assert has.alpha(0) == ((lm, 0.0) if family == "espnet" else (None, 0.0))
    assert has.alpha(2) == (lm, 2.0) and has.alpha(0.7) == (lm, 0.7) and has.alpha(np.float32(0.5)) == (lm, 0.5)
    assert message(lambda: without.alpha(0.3)) == NO_LM
    for bad in (-1.0, float("nan"), float("inf"), True, "0.3"):
        assert message(lambda: has.alpha(bad)) == BAD_ALPHA.format(repr(bad))
        assert message(lambda: without.alpha(bad)) == BAD_ALPHA.format(repr(bad))


def test_nemo_checks_the_models_own_weight_under_its_name():
    lm = toy_lm("nemo")
    assert message(lambda: Nemo(lm=lm, alpha=-1).alpha(None)) == "model.ngram_lm_alpha must be a finite number >= 0, not -1"
    assert message(lambda: Nemo(alpha=True).alpha(None)) == "model.ngram_lm_alpha must be a finite number >= 0, not True"
    m = Nemo(lm=lm, alpha=0.25)
    m.graphs(None, 2)                                                      # transcribe_batch has no keyword: the model's own pair
    assert m.calls[-1][2] == (lm, 0.25)


@pytest.mark.parametrize("family", ("nemo", "k2"))
def test_a_weight_for_a_search_that_cannot_fuse(family):
    lm = toy_lm(family)
    m = MODEL[family]("greedy_batch", lm=lm, alpha=0.25)
    want = (NEMO_LM if family == "nemo" else K2_LM).format("'greedy_batch'")
    assert message(lambda: m.alpha(0.5)) == want
    assert m.alpha(0) == (None, 0.0)                                       # without the LM: nothing to refuse
    if family == "nemo":
        assert message(lambda: m.alpha(None)) == want
    else:
        assert m.alpha(None) is None                                       # left to the runtime's plan


@pytest.mark.parametrize("family", ("k2", "espnet"))
def test_the_forwarded_options(family):
    """`ngram_lm_alpha`, `token_scores`, `resample` and `nbest` of K2Model / EspnetModel are the runtime model's, checked on the way in"""
    m = MODEL[family]().model
    m.ngram_lm_alpha = 2
    assert m.am.ngram_lm_alpha == 2.0 and isinstance(m.am.ngram_lm_alpha, float) and m.ngram_lm_alpha == 2.0
    for bad in (-1, float("nan"), True, None):
        assert message(lambda: setattr(m, "ngram_lm_alpha", bad)) == BAD_ALPHA.format(repr(bad))
    m.token_scores = 1
    assert m.am.token_scores is True and m.token_scores is True
    m.resample = "device"
    assert m.am.resample == "device" and m.resample == "device"
    with pytest.raises(ValueError, match="resample"):
        m.resample = "gpu"
    m.am.nbest, m.am.resample_batch = 3, lambda waveforms, rates: ("resampled", waveforms, rates)
    assert m.nbest == 3 and m.resample_batch([WAVE], [8000]) == ("resampled", [WAVE], [8000])
    uploads = []
    m.am.ngram_set = uploads.append
    lm = toy_lm(family)
    m.ngram_lm = lm                                                        # checked against the model and uploaded once
    assert m.am.ngram_lm is lm and m.ngram_lm is lm and uploads == [lm]
    cfg = CFG[family]
    wrong = NL.build({(10,): (-0.5, 0.0)}, cfg.vocab_size, cfg.blank_id, cfg.n_logits + 3)
    assert message(lambda: setattr(m, "ngram_lm", wrong)) == f"the n-gram LM was built for {cfg.n_logits + 3} logits, the model has {cfg.n_logits}"
    assert m.am.ngram_lm is lm and uploads == [lm]
    if family == "k2":
        m.am.nbest_plan = lambda n: ("planned", n)
        m.nbest = 2
        assert m.am.nbest == ("planned", 2)
