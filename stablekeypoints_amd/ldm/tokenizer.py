"""CLIP byte-pair tokenizer: the `model.tokenizer` of the reference's sampling entry (ptp_utils.py:436-439), written here so that the
product imports neither `transformers` nor `tokenizers`.

    tok = CLIPTokenizer.from_dir("<checkpoint>/tokenizer")        # vocab.json, merges.txt, pad token from the json files beside them
    tok = CLIPTokenizer.byte_level()                               # synthetic architectures: built-in vocabulary, no merges
    tok(["a photo"], padding="max_length", max_length=77, return_tensors="pt").input_ids        # int64 [n, 77]

Processing: lower-casing, whitespace collapse, the CLIP split pattern (contractions, letter runs, single digits, punctuation
runs), the byte-to-unicode table, merges by rank with `</w>` on a word's last symbol, BOS in front and EOS behind.  A text longer
than `max_length` is cut so that EOS stays last.  Padding uses the checkpoint's pad id: EOS for SD-1.x, "!" (id 0) for SD-2.x and
SDXL's second tokenizer -- where, as in the original, a "!" typed in a prompt is that special token too and never merges.

The Unicode classes of the split pattern come from `regex` when it imports; otherwise an `re` pattern that agrees with it on
ASCII text.  There is no `ftfy` and no Unicode normalisation: NON-ASCII TEXT IS BEST EFFORT (its bytes are always encodable, but
the split into words may differ from the original tokenizer's).

The built-in byte-level vocabulary has 514 ids and is deterministic: the 256 byte symbols (ids 0-255, in byte order), their 256
`</w>` forms (256-511), BOS 512, EOS 513 (also the pad).  It lets prompts work on synthetic models in tests and tools.
"""
from __future__ import annotations

import json
import os
import re
from typing import Dict, List, Optional, Sequence, Tuple

import torch

BOS, EOS = "<|startoftext|>", "<|endoftext|>"
BYTE_VOCAB, BYTE_BOS, BYTE_EOS = 514, 512, 513          # the built-in byte-level vocabulary: its size and the two ids behind the symbols
_SPLIT_UNICODE = r"<\|startoftext\|>|<\|endoftext\|>|'s|'t|'re|'ve|'m|'ll|'d|[\p{L}]+|[\p{N}]|[^\s\p{L}\p{N}]+"
_SPLIT_ASCII = r"<\|startoftext\|>|<\|endoftext\|>|'s|'t|'re|'ve|'m|'ll|'d|[^\W\d_]+|\d|(?:[^\s\w]|_)+"


def _split_pattern():
    try:
        import regex
        return regex.compile(_SPLIT_UNICODE, regex.IGNORECASE)
    except ImportError:
        return re.compile(_SPLIT_ASCII, re.IGNORECASE)


def bytes_to_unicode() -> Dict[int, str]:
    """The byte -> printable character table of the GPT-2 / CLIP vocabularies."""
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(0xA1, 0xAC + 1)) + list(range(0xAE, 0xFF + 1))
    cs = bs[:]
    n = 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return {b: chr(c) for b, c in zip(bs, cs)}


class Encoding(dict):
    """What a call returns: `.input_ids` (and `["input_ids"]`)."""

    @property
    def input_ids(self):
        return self["input_ids"]


class CLIPTokenizer:
    model_max_length = 77

    def __init__(self, vocab: Dict[str, int], merges: Sequence[Tuple[str, str]], pad_token: str = EOS):
        self.encoder = dict(vocab)
        self.merges = [tuple(m) for m in merges]
        self.ranks = {m: i for i, m in enumerate(self.merges)}
        for t in (BOS, EOS, pad_token):
            if t not in self.encoder:
                raise ValueError(f"CLIP tokenizer: the vocabulary has no {t!r}")
        self.pad_token = pad_token
        self.bos_token_id, self.eos_token_id, self.pad_token_id = self.encoder[BOS], self.encoder[EOS], self.encoder[pad_token]
        self._bytes = bytes_to_unicode()
        self._pat = _split_pattern()
        self._cache = {BOS: BOS, EOS: EOS}

    # ---- construction -------------------------------------------------------------------------------------------------------
    @classmethod
    def byte_level(cls):
        table = bytes_to_unicode()
        vocab = {table[b]: b for b in range(256)}
        vocab.update({table[b] + "</w>": 256 + b for b in range(256)})
        vocab[BOS], vocab[EOS] = BYTE_BOS, BYTE_EOS
        return cls(vocab, [], EOS)

    @classmethod
    def from_dir(cls, path: str):
        """`vocab.json` + `merges.txt`; the pad token from `special_tokens_map.json` or `tokenizer_config.json` (EOS when neither
        names one).  A missing file raises and names it."""
        vp, mp = os.path.join(path, "vocab.json"), os.path.join(path, "merges.txt")
        for p in (vp, mp):
            if not os.path.isfile(p):
                raise FileNotFoundError(f"CLIP tokenizer: {p} is missing")
        with open(vp, encoding="utf-8") as f:
            vocab = json.load(f)
        with open(mp, encoding="utf-8") as f:
            lines = f.read().split("\n")
        if lines and lines[0].startswith("#version"):
            lines = lines[1:]
        merges = [tuple(l.split()) for l in lines if l.strip()]
        pad = None
        for name in ("special_tokens_map.json", "tokenizer_config.json"):
            p = os.path.join(path, name)
            if pad is None and os.path.isfile(p):
                with open(p, encoding="utf-8") as f:
                    pad = json.load(f).get("pad_token")
                if isinstance(pad, dict):
                    pad = pad.get("content")
        return cls(vocab, merges, pad or EOS)

    def save(self, path: str):
        """Write the three files `from_dir` reads."""
        os.makedirs(path, exist_ok=True)
        with open(os.path.join(path, "vocab.json"), "w", encoding="utf-8") as f:
            json.dump(self.encoder, f, ensure_ascii=False)
        with open(os.path.join(path, "merges.txt"), "w", encoding="utf-8") as f:
            f.write("#version: 0.2\n" + "".join(f"{a} {b}\n" for a, b in self.merges))
        with open(os.path.join(path, "special_tokens_map.json"), "w", encoding="utf-8") as f:
            json.dump({"bos_token": BOS, "eos_token": EOS, "pad_token": self.pad_token, "unk_token": EOS}, f)

    def __len__(self):
        return len(self.encoder)

    # ---- encoding -----------------------------------------------------------------------------------------------------------
    def _bpe(self, token: str) -> str:
        if token in self._cache:
            return self._cache[token]
        word = tuple(token[:-1]) + (token[-1] + "</w>",)
        while len(word) > 1:
            pairs = set(zip(word[:-1], word[1:]))
            best = min(pairs, key=lambda p: self.ranks.get(p, float("inf")))
            if best not in self.ranks:
                break
            a, b = best
            new, i = [], 0
            while i < len(word):
                if i < len(word) - 1 and word[i] == a and word[i + 1] == b:
                    new.append(a + b)
                    i += 2
                else:
                    new.append(word[i])
                    i += 1
            word = tuple(new)
        out = self._cache[token] = " ".join(word)
        return out

    def tokenize(self, text: str) -> List[str]:
        """Symbols of `text`.  A pad token that is a symbol of its own ("!" in the SD-2.x files) is a special token like BOS and
        EOS: as in the original tokenizer every occurrence in the text is cut out and stands for itself (id 0), it never merges."""
        text = " ".join(text.split()).lower()
        pieces = [text] if self.pad_token in (BOS, EOS) else text.split(self.pad_token)
        out = []
        for n, piece in enumerate(pieces):
            if n:
                out.append(self.pad_token)
            for tok in self._pat.findall(piece):
                tok = "".join(self._bytes[b] for b in tok.encode("utf-8"))
                out.extend(self._bpe(tok).split(" "))
        return out

    def encode(self, text: str, max_length: Optional[int] = None) -> List[int]:
        """BOS + ids + EOS, cut to `max_length` with EOS kept last; a symbol outside the vocabulary encodes as EOS (the
        vocabularies' unknown token)."""
        ids = [self.bos_token_id] + [self.encoder.get(t, self.eos_token_id) for t in self.tokenize(text)] + [self.eos_token_id]
        if max_length is not None and len(ids) > max_length:
            ids = ids[:max_length - 1] + [self.eos_token_id]
        return ids

    def __call__(self, text, padding="max_length", max_length: Optional[int] = None, truncation=True, return_tensors=None):
        """`padding`: "max_length" (pad every row to `max_length`), True / "longest" (to the longest row), False / "do_not_pad".
        `return_tensors="pt"`: `.input_ids` is an int64 tensor [n, L] (the rows must then have one length)."""
        texts = [text] if isinstance(text, str) else list(text)
        max_length = self.model_max_length if max_length is None else int(max_length)
        if max_length < 2:
            raise ValueError("max_length must hold BOS and EOS")
        rows = [self.encode(t, max_length if truncation else None) for t in texts]
        if padding == "max_length":
            width = max_length
        elif padding in (True, "longest"):
            width = max(len(r) for r in rows)
        elif padding in (False, None, "do_not_pad"):
            width = 0
        else:
            raise ValueError(f"padding={padding!r} is not built (max_length, longest, do_not_pad)")
        rows = [r + [self.pad_token_id] * (width - len(r)) for r in rows]
        if return_tensors == "pt":
            rows = torch.tensor(rows, dtype=torch.long)
        elif return_tensors is not None:
            raise ValueError("return_tensors: 'pt' or None")
        elif isinstance(text, str):
            rows = rows[0]
        return Encoding(input_ids=rows)
