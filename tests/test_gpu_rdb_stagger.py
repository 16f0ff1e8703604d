"""GPU: the staggered fused dense-block kernel (rdb_f16x2_kernel with NESR_RDB_LAG: MFMA waves 4..7 take each step's
barrier part of a step late, the DMA waves fetch conv1..conv4 two steps ahead) against the per-layer launches of the same
arithmetic (NESR_RDB_FUSE=0), bit for bit, on the tile shapes at which the two halves of a workgroup differ: waves 4..7
without a row or with one row only, a narrow second tile column, second tile rows of 1 and 5 rows, and a tile with all
eight neighbours.  One RRDB (num_block=1) = three dense blocks, the third with the second residual; three forwards per
case, so that the epochs of the progress words advance.

Reference semantics: the dense block of basicsr's RRDBNet (restated in oracle/rrdbnet_ref.py); the per-layer path is
checked against that oracle in test_gpu_rdb_fused.py."""
import pytest
import torch

from tests.rdb_pair import launches as _launches, net as _net

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nets(cuda_device):
    """(per-layer, fused) per scale: built once, shared by the cases."""
    from neural_enhanced_super_resolution_amd.synth import synthetic_state_dict
    out = {}
    for scale in (2, 4):
        sd = synthetic_state_dict(seed=0, num_in_ch=3, scale=scale, num_block=1)
        out[scale] = (_net(sd, 1, False, scale=scale), _net(sd, 1, True, scale=scale))
    return out


# internal size = what the dense blocks see: the x2 form unshuffles (input = 2 x internal), the x4 form does not
@pytest.mark.parametrize("scale,internal", [
    (2, (8, 32)),         # one whole tile, no neighbour
    (2, (4, 36)),         # waves 4..7 without a row; the second tile column is 4 pixels wide
    (2, (5, 36)),         # of waves 4..7 only wave 4 has a row
    (2, (9, 32)),         # a second tile row of 1 row
    (2, (13, 40)),        # a second tile row of 5 rows, second tile column 8 pixels wide
    (2, (24, 96)),        # 3 x 3 tiles: the centre tile polls eight neighbours under the two-step fetch lead
    (4, (12, 40)),        # x4 form
])
def test_staggered_fused_equals_per_layer_bitwise(cuda_device, nets, scale, internal):
    per_layer, fused = nets[scale]
    f = 2 if scale == 2 else 1
    x = torch.rand(1, 3, f * internal[0], f * internal[1], generator=torch.Generator().manual_seed(5)).to(cuda_device)
    want = per_layer(x)
    per_layer.check_status()
    for i in range(3):
        got = fused(x)
        fused.check_status()
        assert torch.equal(got, want), (i, (got - want).abs().max().item())
    # the fused kernel is what ran: one launch per dense block instead of five
    n_fused, n_per_layer = _launches(fused, x), _launches(per_layer, x)
    assert n_per_layer - n_fused == 12, (n_fused, n_per_layer)
