"""GPU: rdb_bf16_strip_kernel's outer loop -- SEVERAL items on one workgroup -- on small images.

A workgroup walks a list of items (strip_schedule): between two of them it re-zeroes its LDS windows, walks the window bases
again to the item's first position, takes the next mailboxes (they belong to the unit, not to the workgroup) and may have to
wait for a neighbour that is still busy with an earlier item.  On a device of 256 compute units the suite's small batches never
queue anything (one item per workgroup: test_strip_schedule_host.py), so these tests plan for FEWER workgroups than the device has
(NESR_STRIP_CUS, read when the context is created; the launch is an ordinary launch of that many workgroups).

In every test the reference of an image is the same image evaluated alone on a context with the default packing -- one item per
workgroup, the path test_gpu_rdb16_block.py and test_gpu_rrdb_emu16.py hold per value -- equality is torch.equal, the route
is asserted by the dense blocks' launch counter (3 per RRDB on the strip route, 15 per layer), and what a test says about its
own plan (items per workgroup, makespan, segments) is asserted through nesr_strip_schedule, the packer the context runs.  bf16
and f16, the x2 and the x4 model (x2: input sizes doubled, the trunk sizes are the same).

The time of a position that DESIGN.md quotes is printed by test_crowd_of_small_images_on_few_workgroups and
test_queue_longer_than_the_old_cutoff (the context's event timer brackets the dense blocks of a forward only)."""
import contextlib
import os

import numpy as np
import pytest
import torch

from tests import rdb16_block as B
from tests import strip_plan as SP

pytestmark = pytest.mark.gpu

DTYPES = ["bf16", "f16"]
KEYS = ("NESR_STRIP", "NESR_STRIP_CUS", "NESR_STRIP_SEG")


@contextlib.contextmanager
def _env(cus=None, seg=None):
    """NESR_STRIP=1 and the two packing switches (None: unset = the default packing) while contexts are created."""
    old = {k: os.environ.get(k) for k in KEYS}
    for k, v in zip(KEYS, ("1", cus, seg)):
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = str(v)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


_nets, _sds = {}, {}


def _net(scale, dtype, nb, cus=None, seg=None):
    """As test_gpu_strip.py's _net: the context is created now, under the switches.  One net per setting for the process."""
    key = (scale, dtype, nb, cus, seg)
    if key not in _nets:
        from neural_enhanced_super_resolution_amd import RRDBNet
        from neural_enhanced_super_resolution_amd.synth import synthetic_state_dict
        if (scale, nb) not in _sds:
            _sds[(scale, nb)] = synthetic_state_dict(seed=0, num_in_ch=3, scale=scale, num_block=nb)
        with _env(cus, seg):
            net = RRDBNet(3, 3, scale=scale, num_block=nb, compute_dtype=dtype)
            net.load_state_dict(_sds[(scale, nb)])
            net.eval().to("cuda:0")
            net.size_independent = True
            u = net.unshuffle
            net(torch.zeros(1, 3, 4 * u, 4 * u, device="cuda:0"))
            net.check_status()
        net.set_kernel_timing("cuda:0", True)
        net.kernel_time()
        _nets[key] = net
    return _nets[key]


def _device_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _ragged(net, imgs):
    """forward_ragged of CPU images [1, 3, h, w] -> (their outputs on the CPU, dense-block launches, ms of the dense blocks)."""
    sizes = [tuple(im.shape[-2:]) for im in imgs]
    H, W = max(s[0] for s in sizes), max(s[1] for s in sizes)
    x = torch.full((len(imgs), 3, H, W), 3.0, device="cuda:0")          # what lies outside an image must not matter
    for j, im in enumerate(imgs):
        x[j, :, :sizes[j][0], :sizes[j][1]] = im[0].to("cuda:0")
    net.kernel_time()
    out = net.forward_ragged(x, sizes)
    net.check_status()
    ms, launches, _ = net.kernel_time()
    s = net.out_scale()
    return [out[j:j + 1, :, :h * s, :w * s].cpu() for j, (h, w) in enumerate(sizes)], launches, ms


_images, _alone = {}, {}


def _inputs(name, trunk, u):
    """The batch's images (input size = trunk size * u), drawn once per (batch, u)."""
    if (name, u) not in _images:
        g = torch.Generator().manual_seed(17 + u)
        _images[(name, u)] = [torch.rand(1, 3, h * u, w * u, generator=g) for h, w in trunk]
    return _images[(name, u)]


def _reference(name, trunk, j, scale, dtype, nb):
    """Image j of the batch alone on the default packing: one item per workgroup, asserted."""
    key = (name, j, scale, dtype, nb)
    if key not in _alone:
        net = _net(scale, dtype, nb)
        plan = SP.schedule([trunk[j]], _device_cus(), 0)
        assert plan.applies and plan.most_items_per_workgroup() == 1, (trunk[j], plan.makespan)
        out, launches, _ = _ragged(net, [_inputs(name, trunk, net.unshuffle)[j]])
        assert launches == 3 * nb
        _alone[key] = out[0]
    return _alone[key]


def _same(got, want, what):
    assert got.shape == want.shape and torch.equal(got, want), (what, int((got != want).sum()), float((got - want).abs().max()))


# ------------------------------------------------------------------------------------------------------------ 1. crowd
@pytest.mark.parametrize("seg", [-1, 0, 2])
@pytest.mark.parametrize("cus", [4, 7])
@pytest.mark.parametrize("scale", [2, 4])
@pytest.mark.parametrize("dtype", DTYPES)
def test_crowd_of_small_images_on_few_workgroups(cuda_device, dtype, scale, cus, seg):
    """12 ragged images of 13 .. 57 rows and 9 .. 48 columns on 4 and 7 workgroups: up to 8 / 4 items per workgroup (16 / 8 in row
    segments of 2 positions), one-strip images among them, waits of up to 18 positions for a neighbour that is busy with an
    earlier item.  Every image equals itself alone; so it does in another slot order and in a subset; a second call repeats."""
    nb, trunk = 2, SP.crowd()
    plan = SP.schedule(trunk, min(cus, _device_cus()), seg)
    SP.check(plan, trunk, min(cus, _device_cus()))
    assert plan.applies and plan.most_items_per_workgroup() >= (4 if cus == 4 else 2), plan.most_items_per_workgroup()
    assert (max(plan.segments().values()) > 1) == (seg == 2), plan.segments()
    assert 0 < plan.max_wait <= 18, f"max_wait {plan.max_wait}: somebody must wait for a busy neighbour in this plan"
    net = _net(scale, dtype, nb, cus, seg)
    imgs = _inputs("crowd", trunk, net.unshuffle)
    full, launches, ms = _ragged(net, imgs)
    assert launches == 3 * nb, f"{launches} dense-block launches: the batch did not run the strip kernel"
    print(f"crowd {dtype} x{scale} cus {cus} seg {seg}: makespan {plan.makespan}, at most {plan.most_items_per_workgroup()} items per workgroup, "
          f"max_wait {plan.max_wait}: {1e3 * ms / (launches * plan.makespan):.1f} us per position")
    for j in range(len(trunk)):
        _same(full[j], _reference("crowd", trunk, j, scale, dtype, nb), (trunk[j], "in the crowd"))
    again, _, _ = _ragged(net, imgs)
    for j in range(len(trunk)):
        _same(again[j], full[j], (trunk[j], "second call"))
    perm = [7, 2, 11, 0, 5, 9, 4, 1, 10, 3, 8, 6]
    moved, launches, _ = _ragged(net, [imgs[k] for k in perm])
    assert launches == 3 * nb
    for j, k in enumerate(perm):
        _same(moved[j], full[k], (trunk[k], "another slot order"))
    subset = [10, 3, 6, 1, 8]
    part, launches, _ = _ragged(net, [imgs[k] for k in subset])
    assert launches == 3 * nb
    for j, k in enumerate(subset):
        _same(part[j], full[k], (trunk[k], "a subset"))


# ------------------------------------------------------------------------------------------------------------ 2. past 250
@pytest.mark.parametrize("scale", [2, 4])
@pytest.mark.parametrize("dtype", DTYPES)
def test_queue_longer_than_the_old_cutoff(cuda_device, dtype, scale):
    """64 images of 40 .. 136 rows and 16 .. 64 columns for 4 workgroups: a schedule of 354 positions, up to 45 items on a
    workgroup.  Whether the kernel runs a batch depends on the images' own positions (at most 12 here), not on the schedule's
    length: the batch runs the strip kernel (the rule `makespan < 250` sent it to the per-layer kernels, 15 launches, whose
    bits are not the ones these images have alone)."""
    nb, trunk, cus = 1, SP.long_queue(), 4
    plan = SP.schedule(trunk, min(cus, _device_cus()), 0)
    assert plan.applies and plan.makespan >= 256 and plan.most_items_per_workgroup() >= 32, (plan.makespan, plan.most_items_per_workgroup())
    net = _net(scale, dtype, nb, cus)
    imgs = _inputs("long queue", trunk, net.unshuffle)
    full, launches, ms = _ragged(net, imgs)
    assert launches == 3 * nb, f"{launches} dense-block launches: the batch did not run the strip kernel"
    print(f"long queue {dtype} x{scale}: makespan {plan.makespan}, at most {plan.most_items_per_workgroup()} items per workgroup, max_wait "
          f"{plan.max_wait}: {ms:.2f} ms in {launches} launches, {1e3 * ms / (launches * plan.makespan):.1f} us per position")
    for j in (0, 13, 31, 63):
        _same(full[j], _reference("long queue", trunk, j, scale, dtype, nb), (trunk[j], "in the long queue"))


# ------------------------------------------------------------------------------------------------------------ 3. the tag bound
TAG_SHAPES = dict(zip(("at", "beyond"), B.TAG_SHAPES))
_want = {}


def _exact(hw, r, dtype):
    if (hw, r, dtype) not in _want:
        sd, x0, rrdb_in = B.exact_case(hw, r, False, dtype)
        _want[(hw, r, dtype)] = (sd, x0, rrdb_in, B.expected(sd, x0, r, rrdb_in, dtype))
    return _want[(hw, r, dtype)]


@pytest.mark.parametrize("seg", ["-1", "0"])
@pytest.mark.parametrize("side", list(TAG_SHAPES))
@pytest.mark.parametrize("r", [0, 2])
@pytest.mark.parametrize("dtype", DTYPES)
def test_tag_bound_from_both_sides(cuda_device, dtype, r, side, seg):
    """One dense block of an image of 17 columns -- two strips that exchange tags at every position, the last one included -- and
    256 positions (3068 rows: the last tag is epoch + 255 * 8 + 4 = epoch + 2044, the largest below the next launch's epoch) or
    257 (3080 rows).  The first runs the strip kernel (1 launch), uncut and as the packer cuts it; the second does not apply,
    cut or uncut (5 launches: the packer's segments bring its schedule far below any length, its positions stay 257).  Both are
    the closed form of the exact case, bit for bit (test_rdb16_block_host.py proves these cases exact)."""
    hw = TAG_SHAPES[side]
    cus = _device_cus()
    plan = SP.schedule([hw], cus, int(seg))
    assert SP.npos_of(hw[0]) == SP.TAG_POSITIONS + (side == "beyond") and plan.largest_pos1 == SP.npos_of(hw[0])
    assert plan.applies == (side == "at") and plan.pos1_bound == SP.TAG_POSITIONS
    assert (max(plan.segments().values()) > 1) == (seg == "0")
    sd, x0, rrdb_in, want = _exact(hw, r, dtype)
    net = B.block_net(dtype, "strip", sd, seg)
    img = torch.rand(1, 3, *hw, generator=torch.Generator().manual_seed(hw[0]))
    got, launches = B.run_block(net, img.to(cuda_device), x0, r, rrdb_in)
    assert launches == (1 if side == "at" else 5), f"{launches} launches for {SP.npos_of(hw[0])} positions"
    assert got.shape == want.shape
    assert torch.equal(got, want), B.describe_difference(got, want)


# ------------------------------------------------------------------------------------------------------------ 4. one frame, two batchings
@pytest.mark.parametrize("scale,dtype", [(2, "bf16"), (4, "bf16"), (2, "f16"), (4, "f16")])
def test_one_frame_in_two_batchings(cuda_device, scale, dtype):
    """A 300 x 260 frame as tiles of 48 + 2 * 4 through the tiling wrapper, planned for 4 workgroups: all 42 tiles in one ragged
    batch (ten and more items on every workgroup) against batches of 7.  One arithmetic for every tile, however it is batched."""
    from neural_enhanced_super_resolution_amd import RealESRGANer, RRDBNet
    from neural_enhanced_super_resolution_amd.synth import synthetic_frame, synthetic_state_dict
    sd = synthetic_state_dict(seed=0, num_in_ch=3, scale=scale, num_block=1)
    frame = synthetic_frame(300, 260, seed=4)
    u = 2 if scale == 2 else 1
    batches = SP.tile_batches_u8(300, 260, u, tile=48, tile_pad=4, cap=64)
    assert len(batches) == 1 and len(batches[0]) == 42
    plan = SP.schedule(batches[0], min(4, _device_cus()), 0)
    assert plan.applies and plan.most_items_per_workgroup() > 8, (plan.makespan, plan.most_items_per_workgroup())
    assert all(SP.schedule(b, min(4, _device_cus()), 0).applies for b in SP.tile_batches_u8(300, 260, u, tile=48, tile_pad=4, cap=7))
    outs = []
    with _env(cus=4):          # the wrapper's contexts are created by its first frame
        for cap in (64, 7):
            up = RealESRGANer(scale=scale, model_path={"params_ema": sd}, model=RRDBNet(3, 3, scale=scale, num_block=1, compute_dtype=dtype), tile=48,
                              tile_pad=4, pre_pad=0, half=True, device=cuda_device)
            assert up.model.compute_dtype == dtype and up.model.size_independent and up.model.strip_kernel_active()
            up.ragged_batch = cap
            up.model.set_kernel_timing(cuda_device, True)
            up.model.kernel_time()
            calls0 = up.model.calls
            out, _ = up.enhance(frame)
            calls, launches = up.model.calls - calls0, up.model.kernel_time()[1]
            assert calls == -(-42 // cap) and launches == 3 * calls, (cap, calls, launches)
            outs.append(out)
    assert outs[0].shape == (300 * scale, 260 * scale, 3)
    assert np.array_equal(outs[0], outs[1]), int((outs[0] != outs[1]).sum())
