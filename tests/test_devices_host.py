"""RealESRGANer(devices=...) / NESR_DEVICES without a GPU: parsing and validation, the unchanged one-device state, and the
tile assignment of the in-process multi-device mode (sharded.plan_tiles over the entries of `devices`)."""
import pytest
import torch

from neural_enhanced_super_resolution_amd import RRDBNet, RealESRGANer
from neural_enhanced_super_resolution_amd.realesrganer import parse_devices
from neural_enhanced_super_resolution_amd.sharded import plan_tiles
from neural_enhanced_super_resolution_amd.synth import synthetic_state_dict

# the wrapper's attributes after construction at the parent commit (devices=None must add nothing else)
ONE_DEVICE_STATE = {"scale", "tile_size", "tile_pad", "pre_pad", "mod_scale", "half", "tile_batch", "tile_streams", "ragged_tiles",
                    "ragged_batch", "small_job_tiles", "small_job_streams", "device", "weights_provenance", "model"}


@pytest.fixture
def no_env(monkeypatch):
    monkeypatch.delenv("NESR_DEVICES", raising=False)


def _wrapper(tile=512, tile_pad=10, pre_pad=0, scale=2, **kw):
    sd = synthetic_state_dict(seed=0, num_in_ch=3, scale=scale, num_block=1)
    return RealESRGANer(scale=scale, model_path={"params_ema": sd}, model=RRDBNet(3, 3, scale=scale, num_block=1), tile=tile,
                        tile_pad=tile_pad, pre_pad=pre_pad, half=False, device="cpu", **kw)


def test_parse_keyword(no_env):
    assert parse_devices(None, 8) is None
    assert parse_devices([0, 1, 2], 8) == [0, 1, 2]
    assert parse_devices((3,), 8) == [3]
    assert parse_devices([0, 0, 0], 1) == [0, 0, 0]          # repeats: several contexts on one device
    assert parse_devices("1, 0", 2) == [1, 0]
    for bad in ([], [8], [-1], [0, 99], [0.5], [True], ["0"]):
        with pytest.raises(ValueError):
            parse_devices(bad, 8)


def test_parse_environment(monkeypatch):
    monkeypatch.setenv("NESR_DEVICES", "0,1,1")
    assert parse_devices(None, 2) == [0, 1, 1]
    assert parse_devices([0], 2) == [0]                      # the keyword wins
    monkeypatch.setenv("NESR_DEVICES", "")
    assert parse_devices(None, 2) is None
    monkeypatch.setenv("NESR_DEVICES", " ")
    assert parse_devices(None, 2) is None
    for bad in ("0,x", "0,,1", "2", "0,-1"):
        monkeypatch.setenv("NESR_DEVICES", bad)
        with pytest.raises(ValueError, match="NESR_DEVICES"):
            parse_devices(None, 2)


def test_constructor_validates(no_env, monkeypatch):
    n = torch.cuda.device_count()
    with pytest.raises(ValueError):
        _wrapper(devices=[n + 99])
    with pytest.raises(ValueError):
        _wrapper(devices=[])
    monkeypatch.setenv("NESR_DEVICES", str(n + 99))
    with pytest.raises(ValueError, match="NESR_DEVICES"):
        _wrapper()


def test_neither_set_is_todays_wrapper(no_env):
    up = _wrapper()
    assert up.devices is None and not up._multi()
    assert set(vars(up)) == ONE_DEVICE_STATE | {"devices"}
    assert up.device == torch.device("cpu")
    explicit = _wrapper(devices=None)
    assert {k: v for k, v in vars(explicit).items() if k != "model"} == {k: v for k, v in vars(up).items() if k != "model"}


@pytest.mark.parametrize("hw,tile,pad,scale", [((2160, 3840), 512, 10, 2), ((300, 420), 128, 10, 4), ((310, 430), 128, 10, 4)])
@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0], [0] * 8, [0, 1], [3, 1, 2, 0], list(range(8))])
def test_tile_assignment_is_plan_tiles(no_env, hw, tile, pad, scale, devices):
    up = _wrapper(tile=tile, tile_pad=pad, scale=scale)
    up.devices = devices                                      # (no GPU here: the constructor would refuse the indices)
    h, w = hw
    tiles, shares = up.device_shares(h, w)
    want_tiles, owner = plan_tiles(up, h, w, len(devices))
    assert tiles == want_tiles
    assert len(tiles) == len(up.tile_grid(h, w))
    assert len(shares) == len(devices)
    flat = sorted(i for share in shares for i in share)
    assert flat == list(range(len(tiles))), "every tile exactly once"
    for j, share in enumerate(shares):
        assert share == [i for i, o in enumerate(owner) if o == j]
        assert share == list(range(share[0], share[-1] + 1)) if share else True   # contiguous runs in upstream's order
    if len(tiles) >= len(devices):
        assert all(shares), "every device gets tiles when there are enough"
