"""Edges of the Winograd F(3x3,2x2) weight gradient (wino_wgrad_kernel + reduce_partials_kernel).

Every case calls ops.conv2d_wgrad on a 3x3 / stride 1 / pad 1 layer, requires that the dispatcher served it with the
Winograd kernel and its reduction, compares it with the fp64 reference at WINO_WGRAD_RTOL of the output scale, and
requires a second call on the same inputs to be bit-equal.  The shapes are the smallest at which the stage geometry, the buffer swap and the
right-edge handling of that kernel take another path: one tile; the second lane half outside the row or with one live
tile; a second, nearly empty 16-tile segment; odd widths; the widths at which a 16-byte staging chunk straddles the
right image edge; stages that are all half rows (odd H, last tile row); K-splits with ragged and empty workgroups;
more than one channel block on either side; the zero-padded Cin < 64 route.
"""
import pytest
import torch

from test_conv_routes_gpu import WINO_WGRAD_RTOL, base, close, kernels_of, ref_wgrad, synth_feat

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from asvspoof2021_air_amd import ops
    return ops


def _check(ops, xs, cout, x=None, dy=None, name=None):
    B, cin, H, W = xs
    ws = (cout, cin, 3, 3)
    if x is None:
        x = synth_feat(xs, 1).cuda()
        dy = synth_feat((B, cout, H, W), 6).cuda()
    got, names = kernels_of(lambda: ops.conv2d_wgrad(x, dy, ws, 1, 1))
    served = [base(n) for n in names]
    assert "wino_wgrad_kernel" in served and "reduce_partials_kernel" in served, \
        "%s -> %d was not served by the Winograd weight gradient: %s" % (xs, cout, names)
    again = ops.conv2d_wgrad(x, dy, ws, 1, 1)
    assert torch.isfinite(got).all(), "non-finite weight gradient %s" % (xs,)
    assert torch.equal(got, again), "two calls on the same inputs differ %s" % (xs,)
    err = close(got, ref_wgrad(x, dy, ws, 1, 1), WINO_WGRAD_RTOL, name or "wino wgrad %s -> %d" % (xs, cout))
    print("wino wgrad %s -> %d: rel err %.3g" % (xs, cout, err))


@pytest.mark.parametrize("W", [2, 15, 16, 17, 31, 33, 35, 37, 46])
def test_widths(ops, W):
    _check(ops, (2, 64, 4, W), 64)


@pytest.mark.parametrize("H", [1, 2, 3, 5])
def test_heights(ops, H):
    _check(ops, (2, 64, H, 33), 64)


@pytest.mark.parametrize("wgs", [1, 3, 1 << 20])
def test_k_split(ops, wgs):
    from asvspoof2021_air_amd import _hip
    with _hip.options(WINO_WGRAD_WGS=wgs):
        _check(ops, (3, 64, 5, 40), 64)


@pytest.mark.parametrize("cin,cout", [(128, 64), (64, 128)])
def test_channel_blocks(ops, cin, cout):
    _check(ops, (2, cin, 3, 33), cout)


def test_padded_route(ops):
    _check(ops, (2, 32, 7, 21), 64)


def test_poisoned_surroundings(ops):
    """x and dy are views into larger NaN-filled buffers: nothing outside the tensors may reach an accumulator."""
    xs, cout, guard = (2, 64, 5, 35), 64, 4096

    def inside(shape, seed):
        n = 1
        for v in shape:
            n *= v
        big = torch.full((n + 2 * guard,), float("nan"), device="cuda")
        view = big[guard:guard + n].view(shape)
        view.copy_(synth_feat(shape, seed))
        return big, view

    xbig, x = inside(xs, 1)
    dbig, dy = inside((xs[0], cout, xs[2], xs[3]), 6)
    _check(ops, xs, cout, x, dy, "wino wgrad in NaN surroundings")
    assert torch.isnan(xbig[:guard]).all() and torch.isnan(xbig[-guard:]).all()
    assert torch.isnan(dbig[:guard]).all() and torch.isnan(dbig[-guard:]).all()
