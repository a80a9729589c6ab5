"""Tokenizers: the reference reads `model.tokenizer.ids_to_text` of NeMo's SentencePiece
wrapper (pkg/nemo-asr/src/decode.py:41,47).  Two implementations with that one method (and `text_to_ids`, the
way back, which hotwords need):

  SentencePieceTokenizer   wraps a `tokenizer.model` taken from a .nemo archive
  SyntheticTokenizer       a seeded vocabulary for synthetic-weight runs (no checkpoint here)
"""
import numpy as np

_WS = "▁"


class SentencePieceTokenizer:
    def __init__(self, model_bytes: bytes):
        import sentencepiece as spm
        self._sp = spm.SentencePieceProcessor(model_proto=model_bytes)
        self.vocab_size = self._sp.get_piece_size()

    def ids_to_text(self, ids):
        return self._sp.decode([int(i) for i in ids])

    def ids_to_tokens(self, ids):
        return [self._sp.id_to_piece(int(i)) for i in ids]

    def text_to_ids(self, text):
        """the readings of `text` as token ids, for hotwords (runtime/nemo_hotwords.py): (a) what SentencePiece's own encode gives,
        and, whenever it differs, (b) the reading the word has in the middle of a Japanese sentence, where no U+2581 precedes it:
        a first piece that is exactly U+2581 is dropped, a first piece U+2581 + X becomes X when X is a piece.  [] when the
        vocabulary cannot spell the text (encode gives <unk>) or the text is empty."""
        ids = [int(i) for i in self._sp.encode(text)]
        unk = self._sp.unk_id()
        if not ids or any(i == unk for i in ids):
            return []
        out = [tuple(ids)]
        first = self._sp.id_to_piece(ids[0])
        if first == _WS:
            if len(ids) > 1:
                out.append(tuple(ids[1:]))
        elif first.startswith(_WS):
            x = self._sp.piece_to_id(first[len(_WS):])
            if x != unk and self._sp.id_to_piece(x) == first[len(_WS):]:
                out.append((int(x),) + tuple(ids[1:]))
        return out


class SyntheticTokenizer:
    """`vocab_size` pieces drawn from kana / kanji / punctuation, with SentencePiece's decode
    rule: concatenate pieces, U+2581 -> space, strip the leading space.  Piece 0 is a bare
    U+2581 (decodes to "" on its own and is dropped by decode.py:53), pieces 1..5 are the
    punctuation marks the segmenter looks for (decode.py:9-11)."""

    def __init__(self, vocab_size: int, seed: int = 0):
        rng = np.random.default_rng(seed)
        fixed = [_WS, "。", "、", "?", "!", ","]
        pool = [chr(c) for c in range(0x3041, 0x3097)] + [chr(c) for c in range(0x30A1, 0x30FB)] + \
               [chr(c) for c in range(0x4E00, 0x4E00 + 4096)]
        pieces = list(fixed[:vocab_size])
        seen = set(pieces)
        while len(pieces) < vocab_size:
            n = int(rng.integers(1, 3))
            p = "".join(pool[int(i)] for i in rng.integers(0, len(pool), size=n))
            if rng.random() < 0.1:
                p = _WS + p
            if p not in seen:
                seen.add(p)
                pieces.append(p)
        self.pieces = pieces
        self.vocab_size = vocab_size

    def text_to_ids(self, text):
        """the reading of `text` as token ids, for hotwords: greedy longest match over the pieces (white space -> U+2581);
        [] when a character matches no piece or the text is empty.  One reading: a list of one tuple."""
        if getattr(self, "_index", None) is None:
            self._index = {p: i for i, p in reversed(list(enumerate(self.pieces)))}
            self._longest = max(len(p) for p in self.pieces)
        text = "".join(_WS if c.isspace() else c for c in text.strip())
        ids, k = [], 0
        while k < len(text):
            for n in range(min(self._longest, len(text) - k), 0, -1):
                i = self._index.get(text[k:k + n])
                if i is not None:
                    ids.append(i)
                    k += n
                    break
            else:
                return []
        return [tuple(ids)] if ids else []

    def ids_to_tokens(self, ids):
        return [self.pieces[int(i)] for i in ids]

    def ids_to_text(self, ids):
        text = "".join(self.pieces[int(i)] for i in ids).replace(_WS, " ")
        return text[1:] if text.startswith(" ") else text
