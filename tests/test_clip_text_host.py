"""The CLIP text encoder without a GPU: the restatement of tests/clip_text_ref.py against transformers' own CLIPTextModel in
float64 on every crafted case (the library is the specification: its mask is causal only, its keys come without `text_model.`);
the state dict under both key generations; every named fault fails the case named for it by at least eight tolerances; the spec's
keys, shapes and parameter count at the published configuration; the launch-count formula; checkpoint round trips; the host side of
a context without a device (strict loading, packing, refusals)."""
import ctypes
import json
import math

import pytest
import torch

from neural_enhanced_super_resolution_amd import ClipTextEncoder, _lib, clip_text_state_dict_spec
from neural_enhanced_super_resolution_amd import clip_text as T
from tests import clip_text_cases as C
from tests import clip_text_ref as R


def library_model(cfg):
    transformers = pytest.importorskip("transformers")
    c = R.config(**cfg)
    config = transformers.CLIPTextConfig(vocab_size=c["vocab_size"], hidden_size=c["hidden_size"], intermediate_size=c["intermediate_size"],
                                         num_hidden_layers=c["num_hidden_layers"], num_attention_heads=c["num_attention_heads"],
                                         max_position_embeddings=c["max_position_embeddings"], layer_norm_eps=c["layer_norm_eps"], hidden_act=c["hidden_act"],
                                         projection_dim=8, pad_token_id=1, bos_token_id=C.BOS, eos_token_id=C.EOS)
    return transformers.CLIPTextModel(config).double().eval()


@pytest.mark.parametrize("name", C.NAMES)
def test_restatement_agrees_with_the_library_in_float64(name):
    case = C.by_name(name)
    net = library_model(case.cfg)
    net.load_state_dict({k: v.double() for k, v in case.sd.items()}, strict=True)      # the same keys and shapes
    y64, _ = C.reference(name)
    with torch.no_grad():
        got = net(input_ids=case.ids)[0]
    err = float((got - y64).abs().max())
    print(f"{name}: restatement vs transformers {err:.3e}")
    assert got.shape == y64.shape and err < 1e-9


def test_the_library_masks_causally_and_nothing_else():
    """What the restatement's mask rests on: a later id, a padding id included, never reaches an earlier position."""
    case = C.by_name("prompt_pair")
    net = library_model(case.cfg)
    net.load_state_dict({k: v.double() for k, v in case.sd.items()}, strict=True)
    other = case.ids.clone()
    other[:, 5] = 2
    with torch.no_grad():
        a, b = net(input_ids=case.ids)[0], net(input_ids=other)[0]
    assert torch.equal(a[:, :5], b[:, :5]) and not torch.equal(a[:, 5], b[:, 5]) and not torch.equal(a[:, 6], b[:, 6])


def test_both_key_generations_load():
    case = C.by_name("prompt_pair")
    old = R.old_generation(case.sd, C.POSITIONS)
    assert "text_model.embeddings.position_ids" in old and all(k.startswith("text_model.") for k in old)
    assert list(T.text_state_dict(old)) == list(case.sd) == list(clip_text_state_dict_spec(**case.cfg))
    for sd in (case.sd, old):
        m = ClipTextEncoder(**case.cfg)
        m.load_state_dict(sd)
        assert list(m.state_dict()) == list(case.sd) and all(torch.equal(v, case.sd[k]) for k, v in m.state_dict().items())
    with pytest.raises(RuntimeError, match="Unexpected key"):
        ClipTextEncoder(**case.cfg).load_state_dict(dict(case.sd, **{"text_projection.weight": torch.zeros(8, 40)}))
    with pytest.raises(RuntimeError, match="Missing key"):
        ClipTextEncoder(**case.cfg).load_state_dict({k: v for k, v in old.items() if k != "text_model.final_layer_norm.bias"})


def test_every_fault_has_a_case():
    assert set(C.FAULT_CASE) == set(R.FAULTS) and set(C.FAULT_CASE.values()) <= set(C.NAMES)


@pytest.mark.parametrize("fault", R.FAULTS)
def test_fault_fails_its_case_by_eight_tolerances(fault):
    name = C.FAULT_CASE[fault]
    case = C.by_name(name)
    y64, tol = C.reference(name)
    with torch.no_grad():
        got = R.forward(case.sd, case.ids, torch.float32, fault=fault, **case.cfg)
    err = float((got.double() - y64).abs().max())
    print(f"{fault} on {name}: err {err:.3e}, tol {tol:.3e}, err / tol {err / tol:.1f}")
    assert tol > 0 and err >= 8 * tol


@pytest.mark.parametrize("name", C.NAMES)
def test_cases_are_seeded_and_finite(name):
    case = C.by_name(name)
    assert list(case.sd) == list(R.spec(**case.cfg)) and all(v.dtype == torch.float32 for v in case.sd.values())
    y64, tol = C.reference(name)
    assert tuple(y64.shape) == tuple(case.ids.shape) + (case.cfg["hidden_size"],) and bool(torch.isfinite(y64).all()) and tol > 0
    again = C._build(name)
    assert all(torch.equal(again.sd[k], case.sd[k]) for k in case.sd) and torch.equal(again.ids, case.ids)


def test_shapes_the_cases_reach():
    shapes = {name: tuple(C.by_name(name).ids.shape) for name in C.NAMES}
    assert sorted(s[1] for s in shapes.values()) == [1, 7, 32, 33, 77] and {s[0] for s in shapes.values()} == {1, 2}
    assert shapes["chunk_exact"][1] == R.STREAM_CHUNK and shapes["chunk_plus_one"][1] == R.STREAM_CHUNK + 1 and 77 % R.STREAM_CHUNK == 13
    heads = {(C.by_name(n).cfg["hidden_size"], C.by_name(n).cfg["num_attention_heads"]) for n in C.NAMES}
    assert heads == {(32, 4), (40, 5), (128, 2)} and 40 % 16 == 8 and C.by_name("prompt_pair").cfg["intermediate_size"] % 16 == 8
    assert {C.by_name(n).cfg["num_hidden_layers"] for n in C.NAMES} == {1, 3} and {C.by_name(n).cfg["hidden_act"] for n in C.NAMES} == {"gelu", "quick_gelu"}
    pair = C.by_name("prompt_pair").ids
    assert int(pair[1, 0]) == 0 and int(pair[0, -1]) == C.VOCAB - 1 and pair[0].tolist().count(11) == 2 and pair[1].tolist().count(3) == 3
    full = C.by_name("full_length").ids
    assert full.shape[1] == C.POSITIONS and int((full[0] == C.EOS).sum()) == 77 - 8 and int((full[1] == C.EOS).sum()) == 76


def test_spec_of_the_published_configuration():
    spec = clip_text_state_dict_spec()
    assert spec == R.spec() and list(spec) == list(R.spec())
    assert spec["embeddings.token_embedding.weight"] == (49408, 1024) and spec["embeddings.position_embedding.weight"] == (77, 1024)
    assert spec["encoder.layers.22.mlp.fc1.weight"] == (4096, 1024) and spec["encoder.layers.22.mlp.fc2.weight"] == (1024, 4096)
    assert spec["encoder.layers.0.self_attn.q_proj.bias"] == (1024,) and "encoder.layers.23.layer_norm1.weight" not in spec
    assert "text_projection.weight" not in spec and "embeddings.position_ids" not in spec
    params = sum(math.prod(s) for s in spec.values())
    print(f"published configuration: {len(spec)} tensors, {params} parameters")
    assert len(spec) == 2 + 16 * 23 + 2 and 3.0e8 < params < 3.8e8
    assert T.launches_per_forward() == 187 and T.launches_per_forward(**C.SMALL) == 11


def test_the_spec_is_the_library_s_state_dict():
    case = C.by_name("full_length")
    sd = library_model(case.cfg).state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == dict(clip_text_state_dict_spec(**case.cfg))


def test_configuration_is_checked():
    with pytest.raises(TypeError, match="unknown configuration"):
        clip_text_state_dict_spec(projection_dim=512)
    with pytest.raises(ValueError, match="num_hidden_layers must be positive"):
        clip_text_state_dict_spec(num_hidden_layers=0)


def test_checkpoint_round_trips(tmp_path):
    save_file = pytest.importorskip("safetensors.torch").save_file
    case = C.by_name("prompt_pair")
    folder = tmp_path / "text_encoder"
    folder.mkdir()
    old = R.old_generation(case.sd, C.POSITIONS)
    save_file({k: v.contiguous() for k, v in old.items()}, str(folder / "model.safetensors"))
    (folder / "config.json").write_text(json.dumps(dict(R.config(**case.cfg), architectures=["CLIPTextModel"], projection_dim=512, pad_token_id=1)))
    m = ClipTextEncoder.from_checkpoint(folder)
    assert m.config["hidden_size"] == 40 and m.config["hidden_act"] == "quick_gelu" and m.config["num_hidden_layers"] == 3
    assert all(torch.equal(v, case.sd[k]) for k, v in m.state_dict().items()) and list(m.state_dict()) == list(case.sd)
    torch.save(dict(case.sd), tmp_path / "pytorch_model.bin")
    m2 = ClipTextEncoder.from_checkpoint(tmp_path / "pytorch_model.bin", **case.cfg)
    assert all(torch.equal(v, case.sd[k]) for k, v in m2.state_dict().items())
    with pytest.raises(FileNotFoundError, match="not fetched"):
        ClipTextEncoder.from_checkpoint("stabilityai/stable-diffusion-x4-upscaler")
    with pytest.raises(RuntimeError, match="inference only"):
        m2.train()
    with pytest.raises(RuntimeError, match="ROCm device only"):
        m2(case.ids)
    with pytest.raises(ValueError, match=r"\[n, tokens\]"):
        m2(case.ids[0])
    with pytest.raises(ValueError, match="integers"):
        m2(case.ids.float())


# ---------------------------------------------------------------------------------------------- the library's host side
def create(lib, cfg, device=-1):
    c = T._config(cfg)
    handle = ctypes.c_void_p()
    rc = lib.nesr_clip_text_create(ctypes.byref(handle), device, c["vocab_size"], c["hidden_size"], c["intermediate_size"], c["num_hidden_layers"],
                                   c["num_attention_heads"], c["max_position_embeddings"], float(c["layer_norm_eps"]), str(c["hidden_act"]).encode())
    return rc, handle


def load(lib, handle, key, t):
    t = t.detach().to(torch.float32).contiguous()
    shape = (ctypes.c_int64 * max(t.dim(), 1))(*t.shape)
    return lib.nesr_clip_text_load_weight(handle, key.encode(), ctypes.c_void_p(t.data_ptr()), shape, t.dim())


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return _lib.load()


def test_a_context_without_a_device_loads_strictly(lib):
    case = C.by_name("prompt_pair")
    for sd in (case.sd, R.old_generation(case.sd, C.POSITIONS)):
        rc, h = create(lib, case.cfg)
        assert rc == 0 and lib.nesr_clip_text_num_tensors(h) == len(case.sd)
        assert lib.nesr_clip_text_finalize(h) < 0 and b"missing keys in state_dict (" + str(len(case.sd)).encode() in lib.nesr_last_error()
        for k, v in sd.items():
            assert load(lib, h, k, v.float()) == 0, lib.nesr_last_error()
        assert lib.nesr_clip_text_finalize(h) == 0
        assert load(lib, h, "text_model.text_projection.weight", torch.zeros(8, 40)) == _lib.ERR_ARG and b"text_model.text_projection.weight" in lib.nesr_last_error()
        assert load(lib, h, "final_layer_norm.bias", torch.zeros(41)) == _lib.ERR_ARG and b"size mismatch" in lib.nesr_last_error()
        ids = (ctypes.c_int32 * 7)(*range(7))
        assert lib.nesr_clip_text_encode_f32(h, ids, 1, 7, ctypes.c_void_p(16), 7 * 40, None) < 0 and b"without a device" in lib.nesr_last_error()
        lib.nesr_clip_text_destroy(h)


@pytest.mark.parametrize("field, value, match", [
    ("hidden_act", "relu", "hidden_act"),
    ("hidden_act", "gelu_new", "hidden_act"),
    ("hidden_size", 2048, "hidden_size"),
    ("hidden_size", 36, "num_attention_heads"),                   # a head width of 9
    ("num_attention_heads", 3, "num_attention_heads"),            # 32 is no multiple
    ("num_attention_heads", 8, "num_attention_heads"),            # a head width of 4
    ("intermediate_size", 4100, "intermediate_size"),
    ("layer_norm_eps", 0.0, "layer_norm_eps"),
    ("num_attention_heads", 1, None),                             # 32 as one head: fine
    ("num_attention_heads", 2, None),
])
def test_configurations_the_kernels_do_not_take(lib, field, value, match):
    rc, h = create(lib, dict(C.SMALL, **{field: value}))
    if match is None:
        assert rc == 0
        lib.nesr_clip_text_destroy(h)
        return
    assert rc == _lib.ERR_UNSUPPORTED and h.value is None and match in lib.nesr_last_error().decode()
