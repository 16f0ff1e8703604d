"""Crafted SegFormer cases: tiny non-B0 configurations, weights and inputs built so that one fused stage of csrc/segformer.hip
dominates the logits, each case named for the faults (segformer_ref.FAULTS, MAP_FAULTS) it is there to show.

The context has no single-kernel entry, so a stage is isolated through the ordinary forward: few stages, depth 1 where possible,
and crafted tensors (a LayerNorm that sees rows of variance 1e-4, a BatchNorm with running_var 1e-4, a constant query so that the
score of a key depends on the key alone, ...).  test_segformer_cases_host.py checks on the CPU that the float32 restatement
passes every case and that every fault fails a case named for it by 10 x the tolerance; test_gpu_segformer_cases.py runs the
kernels through the same criterion:

  logits   max |got - f64| <= tol,  tol = 8 x max |f32 CPU restatement - f64|, per case
  map      got == the float64 argmax (lowest index among equals) wherever the float64 top-2 margin is >= 2 tol; at most
           segformer_ref.MAX_THIN of the map is left out

Every input is at most 96 x 128 pixels (`segment` makes its own 512 x 512 image of such a frame).

One fault of the kind has no restatement: the stage-0 patch conv reading its zero-padded K tail (147 -> 160) as data.  The weight
rows there are zero, so whatever finite value is read changes nothing; every case here runs that tail at 7 x 7 or 3 x 3 (27 -> 32).
"""
from __future__ import annotations

import functools
import math

import torch

from tests import segformer_ref as R

KCH = R.KEY_CHUNK


class Case:
    """name; cfg (SegformerConfig fields); sd (seeded state dict, crafted); x (pixel_values [1, 3, h, w] float32) or, for
    via == "segment", frame ([h, w, 3] uint8 ndarray); faults (the faults this case is named for); tie (a, b): classifier rows
    a < b are bit-equal; want_max ("first" | "last" | None): the key chunk that holds every row's largest score."""

    def __init__(self, name, cfg, sd, x=None, frame=None, faults=(), tie=None, want_max=None, note=""):
        self.name, self.cfg, self.sd, self.x, self.frame = name, cfg, sd, x, frame
        self.faults, self.tie, self.want_max, self.note = tuple(faults), tie, want_max, note
        self.via = "segment" if frame is not None else "forward"

    def pixel_values(self):
        return R.preprocess(self.frame) if self.via == "segment" else self.x

    def __repr__(self):
        return self.name


def _cfg(hidden, sr, strides, patch, depths=None, mlp=None, dec=32, labels=5):
    n = len(hidden)
    return dict(num_channels=3, num_encoder_blocks=n, depths=tuple(depths or (1,) * n), sr_ratios=tuple(sr), hidden_sizes=tuple(hidden),
                patch_sizes=tuple(patch), strides=tuple(strides), num_attention_heads=tuple(c // 32 for c in hidden),
                mlp_ratios=tuple(mlp or (4,) * n), decoder_hidden_size=dec, num_labels=labels)


def grid(cfg, h, w):
    """[(gh, gw)] of every stage for an h x w input: a k x k conv of stride s with k // 2 padding."""
    out = []
    for k, s in zip(cfg["patch_sizes"], cfg["strides"]):
        h, w = (h + 2 * (k // 2) - k) // s + 1, (w + 2 * (k // 2) - k) // s + 1
        out.append((h, w))
    return out


def key_counts(cfg, h, w):
    return [(gh // sr) * (gw // sr) for (gh, gw), sr in zip(grid(cfg, h, w), cfg["sr_ratios"])]


# ------------------------------------------------------------------------------------------------ the constructions
def _small_variance():
    """Every LayerNorm of stage 0 sees rows of variance about 1e-4, and so does the BatchNorm (running_var 1e-4): eps 1e-6 for
    1e-5 moves a normalised row by per cents.  Two stages of different, non-square grids and 3 heads in the second: the decode
    head's and the patch convs' faults and the softmax scale show here too."""
    cfg = _cfg(hidden=(32, 96), sr=(2, 1), strides=(4, 2), patch=(7, 3), dec=32, labels=5)
    sd = R.seeded_state_dict(seed=11, **cfg)
    s0, b0 = "segformer.stages.0.", "segformer.stages.0.blocks.0."
    sd[s0 + "patch_embeddings.proj.bias"].zero_()
    sd[s0 + "patch_embeddings.layer_norm.weight"].mul_(0.01)      # the residual stream of stage 0: rows of variance 1e-4
    sd[s0 + "patch_embeddings.layer_norm.bias"].zero_()
    sd[b0 + "attention.sequence_reduction.sequence_reduction.weight"].mul_(0.01)
    sd[b0 + "attention.sequence_reduction.sequence_reduction.bias"].zero_()
    for name in ("attention.o_proj", "mlp.fc2"):                   # what the block adds to the stream stays that small
        sd[b0 + name + ".weight"].mul_(0.01)
        sd[b0 + name + ".bias"].mul_(0.01)
    sd["decode_head.linear_fuse.weight"].mul_(0.01)
    sd["decode_head.batch_norm.running_mean"].mul_(0.01)
    sd["decode_head.batch_norm.running_var"].mul_(1e-4)
    x = 0.01 * R.seeded_input(64, 96, seed=11)                     # the patch conv's rows: variance about 1e-4
    return Case("small_variance", cfg, sd, x=x,
                faults=["ln_eps_" + s for s in R.LN_SITES] + ["bn_eps", "bn_no_var", "softmax_scale_c", "patch_pad_s0", "patch_pad_s1",
                                                              "patch_taps_s0", "patch_taps_s1", "up_align_corners", "up_no_clamp",
                                                              "concat_first_first"],
                note="16x24 and 8x12 tokens, 96 keys; hidden 32 and 96 (3 heads)")


def _gelu_wide():
    """fc1 doubled: the depthwise conv's outputs spread beyond +-3, where tanh-gelu and erf-gelu differ most.  mlp_ratio 1,
    decoder width 256, 256 labels, one stage; an 8 x 16 grid whose border columns hold distinct (random) values."""
    cfg = _cfg(hidden=(32,), sr=(1,), strides=(4,), patch=(7,), mlp=(1,), dec=256, labels=256)
    sd = R.seeded_state_dict(seed=12, **cfg)
    sd["segformer.stages.0.blocks.0.mlp.fc1.weight"].mul_(2.0)
    return Case("gelu_wide", cfg, sd, x=R.seeded_input(32, 64, seed=12), faults=["gelu_tanh", "dw_wrap"],
                note="8x16 tokens, 128 keys; mlp 1; decoder 256; 256 labels")


def _negative_scores():
    """A 16 x 24 grid reduced by sr = 5 (the floor drops a row and four columns): 12 keys, padded to 32 in the kernel.  The query
    is almost the constant u and the key almost -u, so every real score is negative and a padding key that scored 0 would take
    most of the softmax.  Depth 3: the residual runs in place three times.  Hidden 96."""
    cfg = _cfg(hidden=(96,), sr=(5,), strides=(4,), patch=(7,), depths=(3,), mlp=(2,), dec=32, labels=33)
    sd = R.seeded_state_dict(seed=13, **cfg)
    g = torch.Generator().manual_seed(113)
    for j in range(3):
        a = f"segformer.stages.0.blocks.{j}.attention."
        u = 0.53 * torch.sign(torch.randn(96, generator=g))      # |u| = 3 in every head
        sd[a + "q_proj.weight"].mul_(0.1)
        sd[a + "q_proj.bias"].copy_(u)
        sd[a + "k_proj.weight"].mul_(0.3)
        sd[a + "k_proj.bias"].copy_(-u)
    return Case("negative_scores_12_keys", cfg, sd, x=R.seeded_input(64, 96, seed=13), faults=["pad_key_zero", "sr_ceil"],
                note="16x24 tokens, sr 5 -> 3x4 = 12 keys; depth 3; hidden 96; 33 labels")


def _chunked(name, h, w, strides, patch, sr, seed, where):
    """One stage, one head.  The image holds a flat coloured band over the token rows whose keys make up the first or the last key
    chunk, so those keys are nearly one vector; the query is that vector (q_proj's bias, its weight scaled down), so the band's
    keys score highest in every row, by several units.  where == "last": each later chunk raises the running maximum, which is
    what the rescale by alpha exists for."""
    cfg = _cfg(hidden=(32,), sr=(sr,), strides=(strides,), patch=(patch,), mlp=(2,), dec=32, labels=5)
    sd = R.seeded_state_dict(seed=seed, **cfg)
    (gh, gw), = grid(cfg, h, w)
    kw = gw // sr
    keys = (gh // sr) * kw
    px = sr * strides                                              # image rows per key row
    if where == "first":
        band = slice(0, (KCH // kw) * kw)
    else:
        band = slice(math.ceil(((keys - 1) // KCH * KCH) / kw) * kw, keys)
    x = R.seeded_input(h, w, seed=seed)
    rows = slice(band.start // kw * px, min(band.stop // kw * px, h))
    x[:, :, rows] = 0.2 * x[:, :, rows] + torch.tensor([2.0, -1.5, 1.0]).view(1, 3, 1, 1)
    a = "segformer.stages.0.blocks.0.attention."
    sd[a + "q_proj.weight"].mul_(0.25)
    case = Case(f"{name}_max_{where}", cfg, sd, x=x, faults=["no_alpha_rescale", "no_alpha_rescale_sum", "no_alpha_rescale_acc"] if where == "last" else [], want_max=where,
                note=f"{gh}x{gw} tokens, {keys} keys ({-(-keys // KCH)} chunks), the largest scores in the {where} chunk")
    taps = {}
    with torch.no_grad():
        R.segformer_forward(sd, x.double(), taps=taps, **cfg)
    sd[a + "q_proj.bias"].copy_(1.5 * taps["keys"][0][0, 0, band].mean(dim=0).float())
    return case


def scores_of(case):
    """The float64 scaled scores [heads, m, keys] of the first block."""
    taps = {}
    with torch.no_grad():
        R.segformer_forward(case.sd, case.pixel_values().double(), taps=taps, **case.cfg)
    return taps["scores"][0][0]


def max_chunk_share(case):
    """The share of score rows whose maximum lies in the chunk the case wants it in."""
    s = scores_of(case)
    chunk = s.argmax(dim=-1) // KCH
    want = 0 if case.want_max == "first" else (s.shape[-1] - 1) // KCH
    return float((chunk == want).double().mean())


def _wide():
    """Hidden 256 with sr = 2: q alone is one 256-column chunk of the second product; mlp_ratio 8 (K = 2048 in fc2); 8 heads;
    decoder width 256; 16 keys; one label."""
    cfg = _cfg(hidden=(256,), sr=(2,), strides=(4,), patch=(7,), mlp=(8,), dec=256, labels=1)
    sd = R.seeded_state_dict(seed=14, **cfg)
    return Case("wide_256", cfg, sd, x=R.seeded_input(32, 32, seed=14), faults=["softmax_scale_c"],
                note="8x8 tokens, 16 keys; hidden 256 (8 heads), mlp 8, decoder 256, 1 label")


def _three_stages():
    """Three stages from a stride-8 patch embed: 12 x 16, 6 x 8 and 3 x 4 tokens (48 = 32 + 16 rows; 12 < 32), a depth of 3 in
    the middle, mlp ratios 2, 4 and 1."""
    cfg = _cfg(hidden=(32, 64, 96), sr=(2, 1, 1), strides=(8, 2, 2), patch=(7, 3, 3), depths=(1, 3, 1), mlp=(2, 4, 1), dec=64, labels=33)
    sd = R.seeded_state_dict(seed=15, **cfg)
    return Case("three_stages_stride_8", cfg, sd, x=R.seeded_input(96, 128, seed=15),
                faults=["patch_pad_s1", "patch_taps_s1", "concat_first_first", "up_align_corners", "up_no_clamp", "dw_wrap"],
                note="12x16, 6x8, 3x4 tokens; 48, 48, 12 keys; 33 labels")


def _all_negative(labels, seed, tie=None):
    """Through `segment` (the ARGMAX output mode), one stage of stride 8: a 64 x 64 map, 256 keys.  The classifier's weights are
    all negative and so is its bias; ReLU's output is not, so every real logit is negative and a padded label column (zero
    weight, zero bias: logit 0) would win everywhere.  tie (a, b): rows a and b of the classifier are bit-equal and the least
    negative, so the pair leads at most positions and the lowest index must win."""
    cfg = _cfg(hidden=(32,), sr=(4,), strides=(8,), patch=(7,), mlp=(1,), dec=32, labels=labels)
    sd = R.seeded_state_dict(seed=seed, **cfg)
    w, b = sd["decode_head.classifier.weight"], sd["decode_head.classifier.bias"]
    w.copy_(-w.abs())
    b.copy_(-0.5 - b.abs())
    if tie:
        w[tie[0]].mul_(0.2)
        w[tie[1]].copy_(w[tie[0]])
        b[tie[1]] = b[tie[0]]
    return Case(f"segment_{labels}_labels_all_negative", cfg, sd, frame=R.seeded_frame(96, 128, seed=seed),
                faults=["argmax_pad_label"] + (["argmax_highest_tie"] if tie else []), tie=tie,
                note=f"segment: 64x64 tokens, 256 keys; {labels} label(s)" + (f"; classifier rows {tie[0]} and {tie[1]} bit-equal" if tie else ""))


@functools.lru_cache(maxsize=None)
def cases():
    out = [_small_variance(), _gelu_wide(), _negative_scores(), _wide(), _three_stages()]
    # exactly 256 keys (one full chunk) and 33 labels
    cfg = _cfg(hidden=(32,), sr=(1,), strides=(4,), patch=(7,), mlp=(1,), dec=32, labels=33)
    out.append(Case("keys_256", cfg, R.seeded_state_dict(seed=16, **cfg), x=R.seeded_input(64, 64, seed=16), note="16x16 tokens, 256 keys"))
    for where in ("first", "last"):
        out.append(_chunked("keys_336_stride_2", 96, 128, 2, 3, 3, 17, where))      # 48x64 tokens, sr 3: 16x21 keys, 336 % 32 = 16
        out.append(_chunked("keys_512", 64, 128, 4, 7, 1, 18, where))               # 16x32 tokens: two full chunks
        out.append(_chunked("keys_576", 96, 96, 4, 7, 1, 19, where))                # 24x24 tokens: 256 + 256 + 64
    out += [_all_negative(1, 20), _all_negative(5, 21, tie=(1, 3)), _all_negative(33, 22)]
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def by_name(name):
    return next(c for c in cases() if c.name == name)


# ------------------------------------------------------------------------------------------------ the criterion
@functools.lru_cache(maxsize=None)
def reference(case):
    """(float64 logits, float32 CPU restatement's logits, tol = 8 x max |f32 - f64|), computed once per case."""
    x = case.pixel_values()
    with torch.no_grad():
        l64 = R.segformer_forward(case.sd, x.double(), **case.cfg)
        l32 = R.segformer_forward(case.sd, x, **case.cfg)
    return l64, l32, 8 * float((l32.double() - l64).abs().max())


def logits_error(got, case):
    """(max |got - f64|, tol)."""
    l64, _, tol = reference(case)
    assert tuple(got.shape) == tuple(l64.shape), (tuple(got.shape), tuple(l64.shape))
    return float((got.double().cpu() - l64).abs().max()), tol


def _without(logits, row):
    return torch.cat([logits[:, :row], logits[:, row + 1:]], dim=1)


def map_check(got_map, case, factor=1.0):
    """(excluded, wrong, positions): `got_map` against the float64 argmax, the lowest index among equals, wherever the float64
    top-2 margin is at least 2 tol x factor.  In a case with bit-equal classifier rows (a, b) the margin is that of the logits
    without row b, and b must never be chosen where a leads."""
    l64, _, tol = reference(case)
    lg = l64 if case.tie is None else _without(l64, case.tie[1])
    ref = R.class_map(lg)
    if case.tie is not None:
        ref = ref + (ref >= case.tie[1]).long()
    margin = R.top2_margin(lg) if lg.shape[1] > 1 else torch.full(ref.shape, math.inf, dtype=l64.dtype)
    firm = margin >= 2 * tol * factor
    got_map = torch.as_tensor(got_map).to(torch.int64).cpu()
    assert tuple(got_map.shape) == tuple(ref.shape), (tuple(got_map.shape), tuple(ref.shape))
    return int((~firm).sum()), int(((got_map != ref) & firm).sum()), ref.numel()


def restatement_map(case, logits, fault=None):
    """class_map of the restatement's `logits`; bit-equal classifier rows are made bit-equal here (a CPU gemm may sum two equal
    columns in different orders; the kernel's MFMA columns share one order, which the GPU test asserts on its logits)."""
    if case.tie is not None:
        logits = logits.clone()
        logits[:, case.tie[1]] = logits[:, case.tie[0]]
    return R.class_map(logits, fault=fault)
