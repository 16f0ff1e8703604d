"""GPU: the chained dense-block launch (rdb_f16x2_chain_kernel: a forward's dense blocks as ONE launch, the block boundary a
nine-neighbour wait on the progress words) against the per-layer launches of the same arithmetic (NESR_RDB_FUSE=0), bit for
bit, at the smallest shapes that reach what is new: a centre tile with all eight neighbours and ragged edges, an RRDB
boundary and a wrap of the buffer rotation (6 blocks), a batch of two, the x4 form with an 8-wide last tile column, epochs
that keep rising over 30 forwards, and the launch accounting of both fused routes."""
import os

import pytest
import torch

from tests.rdb_pair import launches

pytestmark = pytest.mark.gpu


def _net(sd, num_block, env, scale=2):
    """RRDBNet on cuda:0 whose context is created with `env` in force; the environment is restored."""
    from neural_enhanced_super_resolution_amd import RRDBNet
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        n = RRDBNet(3, 3, scale=scale, num_block=num_block)
        n.load_state_dict(sd)
        n.eval().to("cuda:0")
        n(torch.zeros(1, 3, 16, 16, device="cuda:0"))
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return n


PER_LAYER = {"NESR_RDB_FUSE": "0"}
CHAINED = {"NESR_RDB_FUSE": "-1", "NESR_RDB_CHAIN": "1"}
PER_BLOCK = {"NESR_RDB_FUSE": "-1", "NESR_RDB_CHAIN": "0"}


def _sd(scale, num_block):
    from neural_enhanced_super_resolution_amd.synth import synthetic_state_dict
    return synthetic_state_dict(seed=0, num_in_ch=3, scale=scale, num_block=num_block)


def _x(shape, seed):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed)).to("cuda:0")


@pytest.fixture(scope="module")
def shape_a(cuda_device):
    """x2 form, 48 x 136 -> 24 x 68 internal = 3 x 3 tiles, the right column 4 wide, the bottom row full; 2 RRDBs = 6 blocks.
    (input, per-layer result, the state dict)"""
    sd = _sd(2, 2)
    x = _x((1, 3, 48, 136), 21)
    want = _net(sd, 2, PER_LAYER)(x).clone()
    return x, want, sd


def test_centre_tile_rrdb_boundary_and_rotation_wrap(shape_a):
    x, want, sd = shape_a
    net = _net(sd, 2, CHAINED)
    got = net(x)
    torch.cuda.synchronize()
    assert net.chain_state() == (1, 6)
    assert torch.equal(got, want)
    net.check_status()


def test_batch_of_two(cuda_device):
    sd = _sd(2, 1)
    x = _x((2, 3, 32, 64), 22)
    want = _net(sd, 1, PER_LAYER)(x)
    net = _net(sd, 1, CHAINED)
    got = net(x)
    assert net.chain_state() == (1, 3)
    assert torch.equal(got, want)
    net.check_status()


def test_x4_form_last_column_eight_wide(cuda_device):
    sd = _sd(4, 2)
    x = _x((1, 3, 16, 40), 23)
    want = _net(sd, 2, PER_LAYER, scale=4)(x)
    net = _net(sd, 2, CHAINED, scale=4)
    got = net(x)
    assert net.chain_state() == (1, 6)
    assert torch.equal(got, want)
    net.check_status()


def test_thirty_forwards_epochs_keep_rising(shape_a):
    x, want, sd = shape_a
    net = _net(sd, 2, CHAINED)
    outs = []
    for i in range(30):
        outs.append(net(x).clone())
        if i % 7 == 6:
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(outs[0], want)
    for i, o in enumerate(outs):
        assert torch.equal(o, outs[0]), i
    net.check_status()


def test_launch_accounting_of_both_fused_routes(shape_a):
    x, want, sd = shape_a
    chained, per_block = _net(sd, 2, CHAINED), _net(sd, 2, PER_BLOCK)
    n_chained, n_per_block = launches(chained, x), launches(per_block, x)
    assert chained.chain_state() == (1, 6)            # one kernel launch behind the six blocks
    assert per_block.chain_state() == (6, 6)
    assert n_chained == n_per_block                   # kernel_time() counts dense blocks per fused route
    per_layer = _net(sd, 2, PER_LAYER)
    assert launches(per_layer, x) - n_chained == 4 * 6
    assert per_layer.chain_state() == (0, 0)
    assert torch.equal(per_block(x), want) and torch.equal(chained(x), want)


def test_frame_with_more_tiles_than_cus_takes_neither_fused_route(cuda_device):
    sd = _sd(2, 1)
    net = _net(sd, 1, CHAINED)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    h = 2 * 8 * (cus // 8 + 1)                           # internal rows x 256 px = more tiles than CUs
    assert ((h // 2 + 7) // 8) * 8 > cus
    n_small = launches(net, torch.rand(1, 3, 64, 64, device=cuda_device))
    assert net.chain_state() == (1, 3)
    n_large = launches(net, torch.rand(1, 3, h, 512, device=cuda_device))
    assert net.chain_state() == (0, 0)
    assert n_large - n_small == 4 * 3, (n_small, n_large)
    net.check_status()
