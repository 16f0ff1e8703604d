"""SegFormer without a GPU: the restatement of tests/segformer_ref.py pinned to ``transformers`` (float64) and its resize to PIL,
the checkpoint's key set under both name generations, the strictness of the loader, the argument checks of
nesr_segformer_create that come before any device, and the thin-margin condition of the GPU criterion for the committed seeds."""
import ctypes
import os

import numpy as np
import pytest
import torch

os.environ.setdefault("HF_HUB_OFFLINE", "1")
os.environ.setdefault("TRANSFORMERS_OFFLINE", "1")

from neural_enhanced_super_resolution_amd import SegFormer, _lib, segformer_state_dict_spec
from neural_enhanced_super_resolution_amd.segformer import new_key
from tests import segformer_cases as C
from tests import segformer_ref as R

RESIZE_CASES, FORWARD_CASES, FRAME_CASES, MAX_THIN = R.RESIZE_CASES, R.FORWARD_CASES, R.FRAME_CASES, R.MAX_THIN


@pytest.mark.parametrize("h,w", [(64, 64), (96, 160)])
def test_restatement_matches_transformers_f64(h, w):
    transformers = pytest.importorskip("transformers")
    cfg = transformers.SegformerConfig(num_labels=150)
    model = transformers.SegformerForSemanticSegmentation(cfg).eval().double()
    sd = R.seeded_state_dict(seed=0)
    assert set(model.state_dict()) == set(sd)
    model.load_state_dict({k: v.double() if v.dtype.is_floating_point else v for k, v in sd.items()})
    x = R.seeded_input(h, w, seed=7).double()
    with torch.no_grad():
        want = model(pixel_values=x).logits
        got = R.segformer_forward(sd, x)
    assert got.shape == want.shape == (1, 150, h // 4, w // 4)
    err = float((got - want).abs().max())
    print(f"restatement vs transformers f64 at {h}x{w}: max |logit diff| = {err:.3e}, max |logit| = {float(want.abs().max()):.2f}")
    assert err <= 1e-10


@pytest.mark.parametrize("name", [c.name for c in C.cases()])
def test_restatement_matches_transformers_f64_on_the_crafted_cases(name):
    """The non-B0 configurations of tests/segformer_cases.py, with their crafted weights and inputs."""
    transformers = pytest.importorskip("transformers")
    case = C.by_name(name)
    model = transformers.SegformerForSemanticSegmentation(transformers.SegformerConfig(**{k: list(v) if isinstance(v, tuple) else v
                                                                                         for k, v in case.cfg.items()})).eval().double()
    assert set(model.state_dict()) == set(case.sd)
    model.load_state_dict({k: v.double() if v.dtype.is_floating_point else v for k, v in case.sd.items()})
    x = case.pixel_values().double()
    with torch.no_grad():
        want = model(pixel_values=x).logits
    got = C.reference(case)[0]
    assert got.shape == want.shape
    err = float((got - want).abs().max())
    print(f"restatement vs transformers f64, {name}: logits {tuple(want.shape)}, max |diff| = {err:.3e}, max |logit| = {float(want.abs().max()):.2f}")
    assert err <= 1e-10


@pytest.mark.parametrize("case", RESIZE_CASES, ids=lambda c: "%dx%d-%dx%d-f%d" % c)
def test_resize_restatement_matches_pil(case):
    Image = pytest.importorskip("PIL.Image")
    h, w, oh, ow, flt = case
    img = R.seeded_frame(h, w, seed=h)
    want = np.asarray(Image.fromarray(img).resize((ow, oh), Image.BILINEAR if flt == R.PIL_BILINEAR else Image.LANCZOS))
    got = R.pil_resize(img, oh, ow, flt)
    assert got.shape == want.shape and np.array_equal(got, want)


def test_segment_resized_matches_reference_lines():
    Image = pytest.importorskip("PIL.Image")
    img = R.seeded_frame(900, 1300, seed=5)
    pil = Image.fromarray(img)                                      # nesr/nesr.py:701-709
    scale = 1024 / max(pil.size)
    pil = pil.resize((int(pil.size[0] * scale), int(pil.size[1] * scale)), Image.LANCZOS)
    want = np.asarray(pil.resize((512, 512), Image.BILINEAR))     # the extractor's resize
    assert np.array_equal(R.segment_resized(img), want)


def test_key_set_and_parameter_count():
    spec = segformer_state_dict_spec()
    assert len(spec) == 208
    params = sum(int(np.prod(s)) for k, s in spec.items() if not k.rsplit(".", 1)[1].startswith(("running_", "num_batches")))
    assert params == 3752694
    model = SegFormer()
    assert list(model.state_dict()) == list(spec)
    assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == dict(spec)
    assert sum(p.numel() for p in model.parameters()) == 3752694


def test_old_names_map_to_new_names():
    spec = segformer_state_dict_spec()
    olds = [R.old_key(k) for k in spec]
    assert len(set(olds)) == len(olds)
    assert "segformer.encoder.block.0.1.attention.self.sr.weight" in olds and "decode_head.linear_c.3.proj.bias" in olds
    assert "segformer.encoder.layer_norm.2.weight" in olds and "segformer.encoder.patch_embeddings.1.layer_norm.bias" in olds
    renamed = sum(o != k for o, k in zip(olds, spec))
    assert renamed == 200          # the 192 encoder tensors and the eight of the four projections; the rest of the head keeps its names
    for old, new in zip(olds, spec):
        assert new_key(old) == new and new_key(new) == new


def test_load_state_dict_takes_either_generation():
    sd = R.seeded_state_dict(seed=3)
    a, b = SegFormer(), SegFormer()
    a.load_state_dict(sd)
    b.load_state_dict(R.to_old_names(sd))
    for (ka, va), (kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert ka == kb and torch.equal(va, vb) and torch.equal(va, sd[ka])
    nbt = "decode_head.batch_norm.num_batches_tracked"
    a.load_state_dict({k: v for k, v in sd.items() if k != nbt})     # accepted and ignored


@pytest.mark.parametrize("old_names", [False, True])
def test_load_state_dict_is_strict(old_names):
    sd = R.seeded_state_dict(seed=3)
    if old_names:
        sd = R.to_old_names(sd)
    key = [k for k in sd if k.endswith("o_proj.weight") or k.endswith("output.dense.weight")][0]
    with pytest.raises(RuntimeError, match="Missing key"):
        SegFormer().load_state_dict({k: v for k, v in sd.items() if k != key})
    extra = dict(sd)
    extra["segformer.stages.0.blocks.0.attention.extra.weight"] = torch.zeros(1)
    with pytest.raises(RuntimeError, match="Unexpected key"):
        SegFormer().load_state_dict(extra)
    both = dict(sd)
    both[new_key(key) if old_names else R.old_key(key)] = sd[key]      # one tensor under both of its names
    with pytest.raises(RuntimeError, match="same tensor"):
        SegFormer().load_state_dict(both)


def test_from_checkpoint_takes_local_files_only(tmp_path):
    with pytest.raises(FileNotFoundError, match="not a local checkpoint"):
        SegFormer.from_checkpoint("nvidia/segformer-b0-finetuned-ade-512-512")
    sd = R.to_old_names(R.seeded_state_dict(seed=4))
    torch.save(dict(sd), tmp_path / "pytorch_model.bin")
    model = SegFormer.from_checkpoint(tmp_path)
    assert torch.equal(model.state_dict()["decode_head.classifier.weight"], sd["decode_head.classifier.weight"])


def test_from_checkpoint_reads_safetensors(tmp_path):
    st = pytest.importorskip("safetensors.torch")
    sd = R.to_old_names(R.seeded_state_dict(seed=4))
    sub = tmp_path / "st"
    sub.mkdir()
    st.save_file({k: v.contiguous() for k, v in sd.items()}, str(sub / "model.safetensors"))
    model = SegFormer.from_checkpoint(sub / "model.safetensors")
    assert torch.equal(model.state_dict()["segformer.stages.3.layer_norm.bias"], sd["segformer.encoder.layer_norm.3.bias"])


def test_forward_refuses_a_host_tensor_and_training():
    model = SegFormer()
    with pytest.raises(RuntimeError, match="no CPU or PyTorch fallback"):
        model(torch.zeros(1, 3, 64, 64))
    with pytest.raises(RuntimeError, match="no CPU or PyTorch fallback"):
        model(torch.zeros(64, 64, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="inference only"):
        model.train()
    with pytest.raises(TypeError, match="unknown configuration"):
        SegFormer(hidden_size=32)


def _create(**over):
    cfg = dict(R.B0)
    cfg.update(over)
    n = cfg["num_encoder_blocks"]
    arr = lambda name: (ctypes.c_int * n)(*cfg[name])      # noqa: E731
    handle = ctypes.c_void_p()
    rc = _lib.load().nesr_segformer_create(ctypes.byref(handle), 0, cfg["num_channels"], n, arr("depths"), arr("sr_ratios"), arr("hidden_sizes"),
                                           arr("patch_sizes"), arr("strides"), arr("num_attention_heads"), arr("mlp_ratios"),
                                           cfg["decoder_hidden_size"], cfg["num_labels"])
    return rc, handle, _lib.load().nesr_last_error().decode()


@pytest.mark.parametrize("over,word", [
    (dict(hidden_sizes=(64, 128, 320, 512)), "head dimension"),                 # B1-B5: heads (1, 2, 5, 8) of 64
    (dict(num_attention_heads=(1, 1, 5, 8)), "head dimension"),
    (dict(depths=(2, 0, 2, 2)), "not positive"),
    (dict(sr_ratios=(8, 4, -2, 1)), "not positive"),
    (dict(num_labels=0), "num_labels"),
    (dict(decoder_hidden_size=0), "decoder_hidden_size"),
    (dict(num_encoder_blocks=0, depths=(), sr_ratios=(), hidden_sizes=(), patch_sizes=(), strides=(), num_attention_heads=(), mlp_ratios=()),
     "num_encoder_blocks"),
])
def test_create_checks_the_configuration_before_any_device(over, word):
    rc, handle, msg = _create(**over)      # no GPU here: reaching the device would be NESR_ERR_HIP, not NESR_ERR_ARG
    assert rc == _lib.ERR_ARG and not handle.value and word in msg, (rc, msg)


@pytest.fixture(scope="module")
def weights():
    return R.seeded_state_dict(seed=0)


def _thin(logits64, logits32):
    tol = 8 * float((logits32.double() - logits64).abs().max())
    return tol, int((R.top2_margin(logits64) < 2 * tol).sum()), logits64[0, 0].numel()


@pytest.mark.parametrize("h,w,seed", FORWARD_CASES)
def test_thin_margins_are_rare_for_the_committed_seeds(weights, h, w, seed):
    x = R.seeded_input(h, w, seed=seed)
    with torch.no_grad():
        l64 = R.segformer_forward(weights, x.double())
        l32 = R.segformer_forward(weights, x)
    tol, thin, n = _thin(l64, l32)
    print(f"{h}x{w}: max |logit| {float(l64.abs().max()):.2f}, f32 CPU vs f64 {tol / 8:.3e}, tolerance {tol:.3e}, thin margins {thin}/{n}, "
          f"classes {len(l64[0].argmax(0).unique())}, f32/f64 argmax differ at {int((l32[0].argmax(0) != l64[0].argmax(0)).sum())}")
    assert 1e-7 < tol / 8 < 1e-3            # float32 rounding of logits of order 10, nothing else
    assert thin <= MAX_THIN * n


@pytest.mark.parametrize("h,w,seed", FRAME_CASES)
def test_thin_margins_are_rare_for_the_committed_frames(weights, h, w, seed):
    x = R.preprocess(R.seeded_frame(h, w, seed=seed))
    assert x.shape == (1, 3, 512, 512) and float(x.abs().max()) < 2.7
    with torch.no_grad():
        l64 = R.segformer_forward(weights, x.double())
        l32 = R.segformer_forward(weights, x)
    tol, thin, n = _thin(l64, l32)
    print(f"frame {h}x{w}: tolerance {tol:.3e}, thin margins {thin}/{n}, classes > 0 at {int((l64[0].argmax(0) > 0).sum())}/{n}")
    assert thin <= MAX_THIN * n
