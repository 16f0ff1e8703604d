"""Crafted cases of the CLIP text encoder: seeded configurations small enough to run in a moment, each built for a shape the kernels
of csrc/clip_text.hip, or the launches around them, can get wrong.  Every tensor is random (tests/clip_text_ref.py:
seeded_state_dict); the vocabulary has 50 ids, of which 49 is the end-of-text id that also pads, and 77 positions.

  one_token       1 id: query 0 has its single key; one query block, one chunk of which 31 keys do not exist
  prompt_pair     n = 2 x 7 ids, hidden 40 with 5 heads of 8 (rows of 48: 8 pad columns), intermediate 72 (rows of 80), 3 layers,
                  quick_gelu; sample 0 is begin, words with a repeated id, end-of-text, padding; sample 1 starts with id 0 and has
                  no padding
  chunk_exact     32 ids: exactly one query block and one key chunk, the diagonal chunk alone
  chunk_plus_one  33 ids, hidden 128 with 2 heads of 64: the second query block has one query, which reads a whole chunk and then
                  one key of its own
  full_length     n = 2 x 77 ids (max_position_embeddings), 3 layers, gelu: three query blocks, the last ragged; a prompt padded
                  from position 9 and the empty prompt (begin, then end-of-text to the end)

`reference(name)` computes the float64 restatement once and shares it; the tolerance of a case is 8 x max |float32 restatement -
float64| and is never written down.
"""
from __future__ import annotations

from collections import namedtuple

import torch

from tests import clip_text_ref as R

Case = namedtuple("Case", "name cfg sd ids")
VOCAB, POSITIONS = 50, 77
BOS, EOS = 48, VOCAB - 1


def layout(hidden, heads, inter, layers, act="gelu"):
    return dict(vocab_size=VOCAB, hidden_size=hidden, intermediate_size=inter, num_hidden_layers=layers, num_attention_heads=heads,
                max_position_embeddings=POSITIONS, hidden_act=act)


SMALL = layout(32, 4, 128, 1)

# which case must expose which fault (tests/test_clip_text_host.py)
FAULT_CASE = {"not_causal": "chunk_plus_one", "causal_excludes_self": "chunk_exact", "padding_masked": "full_length", "quick_gelu_for_gelu": "prompt_pair",
              "final_norm_dropped": "one_token", "positions_from_one": "full_length", "scale_by_hidden_not_head": "chunk_plus_one", "post_norm": "prompt_pair",
              "heads_interleaved": "prompt_pair"}

_cases, _refs = {}, {}


def prompt(words, tokens):
    """begin, the words, end-of-text, then end-of-text as padding to `tokens` ids: what the tokenizer gives (padding='max_length')."""
    ids = [BOS] + list(words) + [EOS]
    return ids + [EOS] * (tokens - len(ids))


def _words(seed, count):
    g = torch.Generator().manual_seed(7000 + seed)
    return torch.randint(1, BOS, (count,), generator=g).tolist()


def _build(name):
    if name == "one_token":
        return Case(name, SMALL, R.seeded_state_dict(51, **SMALL), torch.tensor([[5]]))
    if name == "prompt_pair":
        cfg = layout(40, 5, 72, 3, "quick_gelu")
        return Case(name, cfg, R.seeded_state_dict(52, **cfg), torch.tensor([prompt([11, 7, 11], 7), [0, 3, 44, 3, 3, 17, EOS]]))
    if name == "chunk_exact":
        return Case(name, SMALL, R.seeded_state_dict(53, **SMALL), torch.tensor([prompt(_words(53, 30), 32)]))
    if name == "chunk_plus_one":
        cfg = layout(128, 2, 256, 1)
        return Case(name, cfg, R.seeded_state_dict(54, **cfg), torch.tensor([prompt(_words(54, 31), 33)]))
    if name == "full_length":
        cfg = layout(32, 4, 128, 3)
        return Case(name, cfg, R.seeded_state_dict(55, **cfg), torch.tensor([prompt(_words(55, 7), 77), prompt([], 77)]))
    raise KeyError(name)


NAMES = ("one_token", "prompt_pair", "chunk_exact", "chunk_plus_one", "full_length")


def by_name(name):
    if name not in _cases:
        _cases[name] = _build(name)
    return _cases[name]


def reference(name):
    """(y64, tol): the float64 restatement, and 8 x the float32 restatement's error."""
    if name not in _refs:
        case = by_name(name)
        with torch.no_grad():
            y64 = R.forward(case.sd, case.ids, torch.float64, **case.cfg)
            y32 = R.forward(case.sd, case.ids, torch.float32, **case.cfg)
        _refs[name] = (y64, 8.0 * float((y32.double() - y64).abs().max()))
    return _refs[name]
