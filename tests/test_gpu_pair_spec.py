"""GPU: the kernels of the default f32 form (f16 pairs) against their exact specification on the CPU (tests/pair_spec.py), per
value, at three levels: one layer through the single-layer hook, one dense block through the band entries on both of its
routes (the fused kernel rdb_f16x2.hip and five launches of conv3x3_f16x2.hip), and whole networks.  The bitwise test of the
two routes (test_gpu_rdb_fused.py) compares kernels that share f16x2_common.h; this one compares each with a closed form.

Nothing measured on a kernel is asserted.  With spec64 the specification and the float32 stand-ins (torch's f32 conv, and the
kernels' 16-channel chunk order) computed here on the same input:
  (b)  max |kernel - spec64| <= 4 max |stand-in - spec64|
  (b') per band of rows / columns one pixel of the layer wide: mean |kernel - spec64| <= 4 mean over the image |stand-in - spec64|
  (b") over the image: mean |kernel - spec64| <= 4 mean |stand-in - spec64|
(pair_spec.conditions; test_pair_spec_host.py shows the wrong kernels that each breaks, by 8 and more).  Every test asserts the
kernel that ran, by last_conv_kernel() or by the launch count.  The ratios this file showed on an MI355X are in DESIGN.md, "The
pair specification of the f32 form"."""
import pytest
import torch

from tests.pair_spec import STANDINS, PairRRDBNet, PairSpec, conditions, describe, join, make_case, pair_bytes, pair_values, split
from tests.test_gpu_conv import SHAPES
from tests.test_gpu_rdb_edges import SHAPES as RDB_SHAPES

pytestmark = pytest.mark.gpu


def _threads():
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))


def _judge(tag, got, spec64, spec32, band_px=1):
    fig = conditions(got, spec64, spec32, band_px)
    print(f"pair {tag}: {describe(fig)}")
    assert bool(torch.isfinite(got).all()), tag
    assert fig["b"], f"{tag}: {describe(fig)}"
    assert fig["b_band"], f"{tag}: {describe(fig)}"
    assert fig["b_mean"], f"{tag}: {describe(fig)}"


def _specs(x, w, b, **kw):
    """(spec64, [stand-ins]) of one layer."""
    _threads()
    return PairSpec().one_layer(x, w, b, **kw), [PairSpec(a).one_layer(x, w, b, **kw) for a in STANDINS]


# ------------------------------------------------------------------------------------------------------------ one layer
@pytest.mark.parametrize("lrelu", [False, True])
@pytest.mark.parametrize("cin,cout", SHAPES)
def test_layer_against_the_pair_specification(cuda_device, cin, cout, lrelu):
    """2 x 19 x 37: the tile is 8 x 32, so three tile rows and two tile columns, partial both ways.  The hook's result passes
    the pair store (oneshot_api.cpp: the layer writes its pair map, which is re-joined), so the specification stores too."""
    from neural_enhanced_super_resolution_amd import conv3x3, last_conv_kernel
    x, w, b = make_case(cin, cout, 19, 37, seed=cin * 11 + cout)
    got = conv3x3(x.to(cuda_device), w, b, lrelu=lrelu, dtype="f32-split").cpu()
    assert last_conv_kernel() == "f16-pair"
    _judge(f"layer {cin}->{cout} lrelu {lrelu}", got, *_specs(x, w, b, lrelu=lrelu))


@pytest.mark.parametrize("scale", [1e-3, 1e-5])
@pytest.mark.parametrize("cin,cout", [(64, 32), (192, 64)])
def test_layer_with_small_activations(cuda_device, cin, cout, scale):
    """Activations of 1e-3: the lo halves would be f16 subnormals without their 2^11 scale; of 1e-5: the hi halves are."""
    from neural_enhanced_super_resolution_amd import conv3x3, last_conv_kernel
    x, w, b = make_case(cin, cout, 19, 37, seed=cin * 11 + cout, scale=scale)
    got = conv3x3(x.to(cuda_device), w, b, lrelu=True, dtype="f32-split").cpu()
    assert last_conv_kernel() == "f16-pair"
    _judge(f"layer {cin}->{cout} x{scale:g}", got, *_specs(x, w, b, lrelu=True))


@pytest.mark.parametrize("n,hw", [(1, (5, 33)), (1, (4, 32)), (2, (9, 35))])
@pytest.mark.parametrize("form", ["3x3", "2x2"])
@pytest.mark.parametrize("cin,cout", [(64, 64), (16, 64)])
def test_upsampled_layer_in_both_forms(cuda_device, cin, cout, form, n, hw):
    """Low-res sizes around the 2x2 kernel's tile of 4 x 32 low-res pixels.  The 2x2 form's taps are the library's own fold."""
    from neural_enhanced_super_resolution_amd import conv3x3, last_conv_kernel
    from neural_enhanced_super_resolution_amd.rrdbnet import fold_upconv_weights
    x, w, b = make_case(cin, cout, hw[0], hw[1], seed=cin + hw[1], n=n)
    got = conv3x3(x.to(cuda_device), w, b, lrelu=True, upsample=True, dtype="f32-split", upconv=form).cpu()
    assert last_conv_kernel() == {"3x3": "f16-pair", "2x2": "upconv2x2"}[form]
    assert got.shape == (n, cout, 2 * hw[0], 2 * hw[1])
    _judge(f"up {form} {cin}->{cout} {n}x{hw}", got, *_specs(x, w, b, lrelu=True, upsample=True, upconv=form, folded=fold_upconv_weights(w)))


def test_layer_on_a_large_frame_in_windows(cuda_device):
    """2 x 64->64 x 500 x 509, test_conv3x3_f32_split_big_tile_variant's frame: more workgroups than compute units, so the
    launch without DMA-only waves (the small frames above run the one with them).  The kernel runs the whole frame; the
    specification is local, so it is evaluated on four windows, each cut with a one-pixel halo where the frame goes on."""
    from neural_enhanced_super_resolution_amd import conv3x3, last_conv_kernel
    x, w, b = make_case(64, 64, 500, 509, seed=77)
    got = conv3x3(x.to(cuda_device), w, b, lrelu=True, dtype="f32-split").cpu()
    assert last_conv_kernel() == "f16-pair"
    windows = {"top-left corner": (0, 0, 40, 0, 70), "bottom-right corner, partial tiles": (0, 460, 500, 439, 509),
               "across the 16 x 32 tile seams": (0, 236, 276, 215, 295), "image 1": (1, 100, 140, 300, 370)}
    for what, (i, y0, y1, x0, x1) in windows.items():
        t, l, bt, r = int(y0 > 0), int(x0 > 0), int(y1 < 500), int(x1 < 509)
        s64, s32 = _specs(x[i:i + 1, :, y0 - t:y1 + bt, x0 - l:x1 + r], w, b, lrelu=True)
        cut = lambda v: v[:, :, t:v.shape[2] - bt, l:v.shape[3] - r]      # noqa: E731
        _judge(f"large frame, {what}", got[i:i + 1, :, y0:y1, x0:x1], cut(s64), [cut(v) for v in s32])


# ------------------------------------------------------------------------------------------------------------ one dense block
_block = {}


def _block_nets():
    """(weights, per-layer net, fused net) of one RRDB in the x4 form (internal size = input size), built once."""
    if not _block:
        from neural_enhanced_super_resolution_amd.synth import synthetic_state_dict
        from tests.rdb_pair import net
        sd = synthetic_state_dict(seed=0, num_in_ch=3, scale=4, num_block=1)
        _block["nets"] = (sd, net(sd, 1, False, scale=4), net(sd, 1, True, scale=4))
        for n in _block["nets"][1:]:
            n.set_kernel_timing("cuda:0", True)
    return _block["nets"]


def _block_inputs(hw, kind):
    """(image, x0, the RRDB's input for the third block), the feature maps as float32 tensors that are their own pairs."""
    key = (hw, kind)
    if key not in _block:
        _threads()
        sd = _block_nets()[0]
        g = torch.Generator().manual_seed(hw[0] * 100 + hw[1])
        img = torch.rand(1, 3, *hw, generator=g)
        if kind == "conv_first":
            x0 = join(PairRRDBNet(sd, 4, 1).first(img)).float()
        else:
            x0 = join(split(0.3 * torch.randn(1, 64, *hw, generator=g))).float()
        rrdb_in = join(split(0.3 * torch.randn(1, 64, *hw, generator=g))).float()
        _block[key] = (img, x0, rrdb_in)
    return _block[key]


@pytest.mark.parametrize("kind", ["conv_first", "by hand"])
@pytest.mark.parametrize("r", [0, 1, 2])
@pytest.mark.parametrize("hw", [hw for n, hw in RDB_SHAPES if n == 1] + [(17, 40)])
def test_dense_block_on_both_routes(cuda_device, hw, r, kind):
    """band_begin, a chosen x0 into the block's input buffer (band_set_rows), band_rdb(r), the output buffer read back
    (band_rows): buffer r is the input of block r and buffer (r + 1) % 3 its output; for r = 2 buffer 0 is also the second
    residual, read and overwritten in place -- it gets another tensor than x0, so that residual is checked per value."""
    sd, per_layer, fused = _block_nets()
    img, x0, rrdb_in = _block_inputs(hw, kind)
    h, w = hw
    out = {}
    for route, net, launches in (("per-layer", per_layer, 5), ("fused", fused, 1)):
        net.band_begin(img.to(cuda_device))
        if r == 2:
            net.band_set_rows(0, 0, pair_bytes(rrdb_in))
        net.band_set_rows(r, 0, pair_bytes(x0))
        net.kernel_time()
        net.band_rdb(r)
        raw = net.band_rows((r + 1) % 3, 0, h).cpu()
        net.check_status()
        assert net.kernel_time()[1] == launches, f"the block did not take the {route} route"
        out[route] = pair_values(raw, h, w)
    assert torch.equal(out["fused"], out["per-layer"]), float((out["fused"] - out["per-layer"]).abs().max())
    _threads()
    run = lambda acc: join(PairRRDBNet(sd, 4, 1, accumulate=acc).dense_block(      # noqa: E731
        split(x0), f"body.0.rdb{r + 1}", rrdb_in=split(rrdb_in) if r == 2 else None))
    spec64, spec32 = run(torch.float64), [run(a) for a in STANDINS]
    for route in out:
        _judge(f"block {hw} r {r} x0 {kind} {route}", out[route], spec64, spec32)


# ------------------------------------------------------------------------------------------------------------ the whole network
INPUT = {2: (66, 94), 4: (23, 47)}        # as test_gpu_rrdb_emu16.py: trunk 33 x 47 / 23 x 47
_net_cache = {}


def _network(scale, num_block, num_in_ch=3):
    key = ("net", scale, num_block, num_in_ch)
    if key not in _net_cache:
        from neural_enhanced_super_resolution_amd.synth import synthetic_state_dict
        from tests.rdb_pair import net
        sd = synthetic_state_dict(seed=0, num_in_ch=num_in_ch, scale=scale, num_block=num_block)
        n = net(sd, num_block, True, num_in_ch=num_in_ch, scale=scale)
        n.set_kernel_timing("cuda:0", True)
        _net_cache[key] = (sd, n)
    return _net_cache[key]


def _network_specs(scale, num_block, num_in_ch, x, form):
    """(spec64, [stand-ins]) of the whole network, one per up-conv form; the trunk is computed once for both forms."""
    from neural_enhanced_super_resolution_amd.rrdbnet import fold_upconv_weights
    key = ("spec", scale, num_block, num_in_ch, form)
    if key not in _net_cache:
        _threads()
        sd = _network(scale, num_block, num_in_ch)[0]
        res = []
        for acc in (torch.float64,) + STANDINS:
            fkey = ("feat", scale, num_block, num_in_ch, acc)
            spec = PairRRDBNet(sd, scale, num_block, accumulate=acc, upconv=form, fold=fold_upconv_weights)
            if fkey not in _net_cache:
                _net_cache[fkey] = spec.features(x)
            res.append(spec.tail(_net_cache[fkey]))
        _net_cache[key] = (res[0], res[1:])
    return _net_cache[key]


def _run_network(cuda_device, scale, num_block, num_in_ch, x, form, last):
    sd, net = _network(scale, num_block, num_in_ch)
    net.set_upconv(form)
    net.set_conv_last(last)
    net.kernel_time()
    got = net(x.to(cuda_device)).cpu()
    net.check_status()
    assert net.kernel_time()[1] == 3 * num_block, "the trunk did not run one fused launch per dense block"
    assert net.upconv_state() == form
    return got


@pytest.mark.parametrize("last", ["narrow", "general"])
@pytest.mark.parametrize("form", ["2x2", "3x3"])
@pytest.mark.parametrize("scale,num_block", [(2, 1), (2, 2), (4, 1), (4, 2)])
def test_network_against_the_pair_specification(cuda_device, scale, num_block, form, last):
    """For the pack, conv_first's two stores, conv_body + skip, the up-convs, conv_hr and conv_last (the trunk is judged at the
    block level above).  conv_last's two launch geometries give the same image: one specification for both."""
    x = torch.rand(1, 3, *INPUT[scale], generator=torch.Generator().manual_seed(scale * 100 + num_block))
    got = _run_network(cuda_device, scale, num_block, 3, x, form, last)
    assert got.shape == (1, 3, INPUT[scale][0] * 4 // (2 if scale == 2 else 1), INPUT[scale][1] * 4 // (2 if scale == 2 else 1))
    _judge(f"x{scale}plus num_block {num_block} up {form} last {last}", got, *_network_specs(scale, num_block, 3, x, form), band_px=4)


def test_network_of_12_input_channels(cuda_device):
    """The pipeline's 12-channel form (num_in_ch = 12, scale 4) on x2plus' trunk size."""
    x = torch.rand(1, 12, 33, 47, generator=torch.Generator().manual_seed(412))
    got = _run_network(cuda_device, 4, 1, 12, x, "2x2", "narrow")
    _judge("12 channels, scale 4, num_block 1", got, *_network_specs(4, 1, 12, x, "2x2"), band_px=4)
