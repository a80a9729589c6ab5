"""Generate tests/golden/reference_eval.json from the reference's own
/root/reference/pkg/evaluation/src/utils.py (run in the BUILD container only).  `editdistance` and
`num2words` are not installed, so the import is satisfied with a textbook Levenshtein and a
`num2words` that raises (the sample strings contain no digits); what gets pinned is the reference's
normalisation tables and the CER arithmetic.

    python tests/golden/make_reference_eval_golden.py [hooks]

`hooks` writes tests/golden/reference_eval_hooks.json instead: the reference's own `BaseEvaluator.evaluate` (base.py) run over six
rows with a subclass that records every call of its `_evaluate` / `_evaluate_batch` hooks (the example, positional and keyword
arguments) and answers with the row's `hint`; stored with the rows it returned."""
import importlib.util
import json
import os
import sys
import types

REF = "/root/reference/pkg/evaluation/src/utils.py"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_eval.json")
OUT_HOOKS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_eval_hooks.json")


def lev(a, b):
    prev = list(range(len(b) + 1))
    for i, ca in enumerate(a, 1):
        cur = [i]
        for j, cb in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (ca != cb)))
        prev = cur
    return prev[-1]


def stub_imports():
    ed = types.ModuleType("editdistance")
    ed.eval = lev
    nw = types.ModuleType("num2words")
    nw.num2words = lambda *a, **k: (_ for _ in ()).throw(OverflowError())
    sys.modules["editdistance"], sys.modules["num2words"] = ed, nw


def main():
    stub_imports()
    spec = importlib.util.spec_from_file_location("ref_eval_utils", REF)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    pairs = [("今日は、良い天気ですね。", "今日は良い天気ですね"), ("「ＡＢＣ」と言った！", "abcと言った"),
             ("東京タワーに行きたい", "東京タワーへ行きたいです"), ("はい？", "はい"), ("ｘｙｚ　テスト", "xyz テスト"),
             ("完全に違う文", "まったく別の文章です"), ("同じ", "同じ")]
    cases = [{"reference": r, "prediction": p, "normalized": [m.normalize(r), m.normalize(p)],
              "cer": m.calculate_cer(r, p)} for r, p in pairs]
    with open(OUT, "w", encoding="utf-8") as fp:
        json.dump({"cases": cases}, fp, ensure_ascii=False, indent=0)
    print("wrote", OUT, len(cases))


def hooks():
    stub_imports()
    src = os.path.dirname(REF)
    pkg = types.ModuleType("_ref_eval")
    pkg.__path__ = [src]
    sys.modules["_ref_eval"] = pkg
    spec = importlib.util.spec_from_file_location("_ref_eval.base", os.path.join(src, "base.py"))
    base = importlib.util.module_from_spec(spec)
    sys.modules["_ref_eval.base"] = base
    spec.loader.exec_module(base)
    import datasets
    calls = []

    class Recording(base.BaseEvaluator):
        def _evaluate(self, example, *a, **kw):
            calls.append({"hook": "_evaluate", "example": {k: example[k] for k in example}, "args": list(a), "kwargs": kw})
            return {"prediction": example["hint"]}

        def _evaluate_batch(self, batch, *a, **kw):
            calls.append({"hook": "_evaluate_batch", "example": {k: batch[k] for k in batch}, "args": list(a), "kwargs": kw})
            return {"predictions": [x["hint"] for x in batch["audio"]]}

    hints = ["あいう" if i % 2 else "あ" for i in range(6)]
    rows = [{"audio": {"hint": h}, "hint": h, "text": "あいう"} for h in hints]
    out = Recording(model=object(), dataset=datasets.Dataset.from_list(rows), text_column="text").evaluate(num_gpus=0)
    result = [{k: v for k, v in r.items() if k != "audio"} for r in out]
    with open(OUT_HOOKS, "w", encoding="utf-8") as fp:
        json.dump({"rows": rows, "evaluate_kwargs": {"num_gpus": 0}, "calls": calls, "result": result}, fp, ensure_ascii=False, indent=0)
    print("wrote", OUT_HOOKS, len(calls), "calls")


if __name__ == "__main__":
    if "hooks" in sys.argv[1:]:
        hooks()
    else:
        main()
