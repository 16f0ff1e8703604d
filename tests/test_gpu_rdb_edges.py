"""GPU: the edges of the fused dense-block kernel -- what runs before its first step and after its last one.

Head: the bias table is filled by the MFMA waves (one vector per wave) instead of DMA wave 0, and the abort word is read
with a scalar load behind the first LDS-DMAs.  Tail: conv5's residuals (x0 of the block; in the third block of an RRDB also
the RRDB's input, whose buffer is the block's output buffer) are all loaded before the first wait and all eight lines of a
wave are stored after its last piece.  What can go wrong is gross, not a last bit: a residual read after its in-place
store, a stale or misplaced bias vector, a wait that counts a load too few.  So: fused (NESR_RDB_FUSE=-1) against per-layer
(NESR_RDB_FUSE=0) bit for bit, x4 form (internal size = input size), one RRDB = three dense blocks (second residual
absent, absent, present in place); repeated forwards over two RRDBs (the in-place buffer is reused across RRDBs and
launches); and both paths against the CPU oracle within the f32-class bound of tests/test_gpu_configs.py (5e-5).

Reference semantics: the dense block of basicsr's RRDBNet (restated in oracle/rrdbnet_ref.py)."""
import pytest
import torch

from tests.rdb_pair import net as _net

pytestmark = pytest.mark.gpu

SHAPES = [
    (1, (8, 32)),         # one whole tile
    (1, (5, 19)),         # one partial tile: three inactive rows, invalid columns in both pixel halves
    (1, (9, 33)),         # four tiles, three partial: a single active row, a single valid column
    (1, (24, 96)),        # 3 x 3 tiles: the centre tile has all eight neighbours
    (2, (16, 64)),        # two images of 2 x 2 tiles
]
F32_CLASS = 5e-5          # max abs error against the oracle (tests/test_gpu_configs.py)


_cache = {}


def _nets(num_block):
    """(per-layer net, fused net, CPU oracle) of one set of weights, built once per module run."""
    if num_block not in _cache:
        from neural_enhanced_super_resolution_amd.synth import synthetic_state_dict
        from oracle.rrdbnet_ref import RRDBNetRef
        sd = synthetic_state_dict(seed=0, num_in_ch=3, scale=4, num_block=num_block)
        ref = RRDBNetRef(3, 3, scale=4, num_block=num_block)
        ref.load_state_dict(sd, strict=True)
        ref.eval()
        _cache[num_block] = (_net(sd, num_block, False, scale=4), _net(sd, num_block, True, scale=4), ref)
    return _cache[num_block]


_want = {}


def _oracle(n, hw):
    """The oracle's output for a shape, computed once and shared."""
    key = (n, hw)
    if key not in _want:
        ref = _nets(1)[2]
        x = torch.rand(n, 3, *hw, generator=torch.Generator().manual_seed(11))
        with torch.no_grad():
            _want[key] = (x, ref(x))
    return _want[key]


@pytest.mark.parametrize("n,hw", SHAPES)
def test_fused_equals_per_layer_bitwise_and_both_match_the_oracle(cuda_device, n, hw):
    per_layer, fused, _ = _nets(1)
    x_cpu, want = _oracle(n, hw)
    x = x_cpu.to(cuda_device)
    got_p = per_layer(x)
    per_layer.check_status()
    got_f = fused(x)
    fused.check_status()
    assert got_f.shape == (n, 3, 4 * hw[0], 4 * hw[1])
    err_p = (got_p.cpu() - want).abs().max().item()
    err_f = (got_f.cpu() - want).abs().max().item()
    print(f"{n}x{hw}: max abs error vs oracle per-layer {err_p:.3e} fused {err_f:.3e}")
    assert torch.equal(got_f, got_p), (got_f - got_p).abs().max().item()
    assert err_p < F32_CLASS, err_p
    assert err_f < F32_CLASS, err_f


def test_two_rrdbs_five_forwards_in_a_row(cuda_device):
    """Six dense blocks per forward, five forwards: the buffer that the third block of an RRDB reads and overwrites in
    place is the next RRDB's input and is reused by every later launch and forward."""
    per_layer, fused, _ = _nets(2)
    x = torch.rand(1, 3, 17, 40, generator=torch.Generator().manual_seed(12)).to(cuda_device)      # 3 x 2 tiles, partial row and column
    want = per_layer(x)
    per_layer.check_status()
    first = None
    for _ in range(5):
        got = fused(x).clone()
        fused.check_status()
        if first is None:
            first = got
        assert torch.equal(got, first), (got - first).abs().max().item()
        assert torch.equal(got, want), (got - want).abs().max().item()
