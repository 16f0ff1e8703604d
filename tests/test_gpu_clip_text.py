"""GPU: `ClipTextEncoder.forward` on every crafted case of tests/clip_text_cases.py against the float64 restatement, within the
case's own tolerance (8 x the float32 restatement's error, computed here).  The result is written into the middle of a buffer of
sentinels (the guards are asserted), a second encode on the same context gives the same bits, the two samples of a pair equal two
encodes of one sample each, bit for bit, the launch count is the formula at any n and tokens, and every argument the entry refuses
is refused before anything is launched."""
import ctypes

import pytest
import torch

from neural_enhanced_super_resolution_amd import ClipTextEncoder, _lib
from neural_enhanced_super_resolution_amd.clip_text import KERNEL_GROUPS, launches_per_forward
from tests import clip_text_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 4096
_cache = {}


def model(name):
    if name not in _cache:
        case = C.by_name(name)
        m = ClipTextEncoder(**case.cfg).to(DEV)
        m.load_state_dict(case.sd)
        _cache[name] = m
    return _cache[name]


def guarded_encode(m, ids, n=None, tokens=None, elems=None):
    """nesr_clip_text_encode_f32 into the middle of a buffer of sentinels -> (status, the result on the host or None); the guards
    are asserted, and after a refusal the whole buffer."""
    n, tokens = (ids.shape[0] if n is None else n), (ids.shape[1] if tokens is None else tokens)
    count = ids.numel() * int(m.config["hidden_size"])
    buf = torch.full((GUARD + count + GUARD,), -777.0, dtype=torch.float32, device=DEV)
    host = (ctypes.c_int32 * ids.numel())(*ids.reshape(-1).tolist())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = _lib.load().nesr_clip_text_encode_f32(m._context(torch.device(DEV)), host, n, tokens, ctypes.c_void_p(buf.data_ptr() + 4 * GUARD),
                                               count if elems is None else elems, stream)
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == -777.0).all()) and bool((buf[GUARD + count:] == -777.0).all()), "the entry wrote outside the result it reports"
    if rc != 0:
        assert bool((buf == -777.0).all()), "a refused call launched something"
        return rc, None
    return rc, buf[GUARD:GUARD + count].view(ids.shape[0], ids.shape[1], -1).cpu()


@pytest.mark.parametrize("name", C.NAMES)
def test_encode_against_the_float64_restatement(name):
    m, case = model(name), C.by_name(name)
    y64, tol = C.reference(name)
    rc, got = guarded_encode(m, case.ids)
    assert rc == 0 and got.shape == y64.shape and bool(torch.isfinite(got).all())
    err = float((got.double() - y64).abs().max())
    print(f"{name}: {tuple(y64.shape)}, err {err:.3e}, tol {tol:.3e}, err / tol {err / tol if tol else 0.0:.3f}")
    assert err <= tol
    again = m(case.ids)
    assert again.is_cuda and again.dtype == torch.float32 and torch.equal(again.cpu(), got)      # a repeated encode: the same bits
    assert torch.equal(m(case.ids.to(DEV)).cpu(), got) and torch.equal(m(case.ids.tolist()).cpu(), got)


@pytest.mark.parametrize("name", ["prompt_pair", "full_length"])
def test_a_sample_does_not_depend_on_its_batch(name):
    m, case = model(name), C.by_name(name)
    both = m(case.ids).cpu()
    for i in range(2):
        alone = m(case.ids[i:i + 1]).cpu()
        assert torch.equal(alone[0], both[i]), f"sample {i} alone differs from sample {i} of two"
    assert not torch.equal(both[0], both[1])


@pytest.mark.parametrize("name", ["one_token", "prompt_pair"])
def test_launch_count_is_the_formula_at_any_n_and_tokens(name):
    m, case = model(name), C.by_name(name)
    m.set_kernel_timing(True)
    counts = []
    for n, tokens in ((1, 1), (2, 77), (1, 33)):
        ids = torch.arange(n * tokens).reshape(n, tokens) % C.VOCAB
        m.kernel_time_ms()
        m(ids)
        t = m.kernel_time_ms()
        counts.append(t["launches"])
    m.set_kernel_timing(False)
    assert counts[0] == counts[1] == counts[2] == launches_per_forward(**case.cfg) == 3 + 8 * case.cfg["num_hidden_layers"]
    assert tuple(t["groups"]) == KERNEL_GROUPS and all(v > 0 for v in t["groups"].values())


def test_workspace_grows_and_is_reused():
    case = C.by_name("prompt_pair")
    used, fresh = model("prompt_pair"), ClipTextEncoder(**case.cfg).to(DEV)
    fresh.load_state_dict(case.sd)
    big, small = torch.arange(2 * 77).reshape(2, 77) % C.VOCAB, case.ids[:1, :3]
    y_big, y_small, y_again = used(big).cpu(), used(small).cpu(), used(big).cpu()
    assert torch.equal(y_big, y_again) and torch.equal(y_small, fresh(small).cpu()) and torch.equal(fresh(big).cpu(), y_big)
    assert used.workspace_bytes(2, 77) > used.workspace_bytes(1, 3) > 0


def test_changed_weight_is_picked_up():
    case = C.by_name("one_token")
    m = ClipTextEncoder(**case.cfg).to(DEV)
    m.load_state_dict(case.sd)
    before = m(case.ids).cpu()
    sd = dict(case.sd)
    sd["final_layer_norm.bias"] = sd["final_layer_norm.bias"] + 1.0
    m.load_state_dict(sd)
    assert float((m(case.ids).cpu() - before - 1.0).abs().max()) < 1e-5 and m.calls == 2


def test_arguments_the_encode_refuses_launch_nothing():
    m, case = model("prompt_pair"), C.by_name("prompt_pair")
    lib = _lib.load()
    bad = case.ids.clone()
    bad[1, 4] = C.VOCAB
    for ids, kw, match in ((bad, {}, "id 50 at position 4 of sample 1"),
                           (-case.ids - 1, {}, "outside the table"),
                           (case.ids, dict(n=3, tokens=7), "n is 1 or 2"),
                           (case.ids, dict(n=0, tokens=7), "n is 1 or 2"),
                           (case.ids, dict(n=1, tokens=78), "tokens must be 1 .. 77"),
                           (case.ids, dict(n=2, tokens=0), "tokens must be 1 .. 77"),
                           (case.ids, dict(elems=2 * 7 * 40 - 1), "out_elems"),
                           (case.ids, dict(elems=2 * 7 * 48), "out_elems")):
        rc, got = guarded_encode(m, ids, **kw)
        assert rc == _lib.ERR_ARG and got is None and match in lib.nesr_last_error().decode(), lib.nesr_last_error()
    with pytest.raises(_lib.NesrHipError, match="tokens must be 1 .. 77"):
        m(torch.zeros((1, 78), dtype=torch.int64))
    with pytest.raises(_lib.NesrHipError, match="tokens must be 1 .. 77"):
        m.workspace_bytes(1, 78)
    with pytest.raises(_lib.NesrUnsupportedError, match="hidden_act"):
        ClipTextEncoder(**dict(C.SMALL, hidden_act="relu")).to(DEV)(case.ids[:1] % 40)
