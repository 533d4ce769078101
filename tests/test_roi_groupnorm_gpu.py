"""The per-ROI GroupNorm (+ ReLU) kernels (csrc/groupnorm_roi.hip) through ubteacher.hip against float64, in fp32 and with 16-bit I/O
in both libraries.  Shapes, inputs, the reference and where the tolerance comes from: tests/roi_gn_ref64.py (nothing here is a chosen
number: the bound is 4 x the error of torch's own fp32 CPU group_norm on the same inputs, plus one ulp for a 16-bit output)."""
import pytest
import torch

from tests import roi_gn_ref64 as R64

pytestmark = pytest.mark.gpu

KINDS = ("fp32", "bf16", "fp16")


def select(kind):
    """-> the torch dtype of `kind` after pointing the wrappers at its library"""
    from ubteacher import hip, ops
    ops.set_precision(kind)
    return torch.float32 if kind == "fp32" else hip.h16_dtype()


def run(c, dt):
    """forward (+ the pre-activation when the ReLU is on) and backward of one case on the GPU"""
    from ubteacher import hip
    x, dy, ga, be = c["x"].cuda().to(dt), c["dy"].cuda().to(dt), c["ga"].cuda(), c["be"].cuda()
    y, mean, rstd = hip.groupnorm_roi_fwd(x, ga, be, c["G"], R64.EPS, c["relu"])
    pre = hip.groupnorm_roi_fwd(x.float(), ga, be, c["G"], R64.EPS, False)[0] if c["relu"] else None     # fp32 I/O: the value whose sign is the mask
    dga, dbe = torch.zeros_like(ga), torch.zeros_like(be)
    dx = hip.groupnorm_roi_bwd(dy, x, mean, rstd, ga, be, dga, dbe, c["G"], c["relu"])
    return dict(y=y, dx=dx, dga=dga, dbe=dbe, pre=pre, mean=mean, rstd=rstd)


def check(c, dt, tag):
    got = run(c, dt)
    cells, chans = c["cells"], c["chans"]
    if c["relu"]:
        kc, kch = R64.flipped(got["pre"].cpu(), c["ref"]["pre"], c["C"], c["G"])
        cells, chans = cells | kc, chans | kch
    keep = R64.keep_masks(c, cells, chans)
    bnd = R64.bounds(c, keep)
    assert bool(torch.isfinite(got["mean"]).all()) and bool(torch.isfinite(got["rstd"]).all())
    worst = {}
    for k in ("y", "dx", "dga", "dbe"):
        err = (got[k].double().cpu() - c["ref"][k]).abs()
        assert bool(torch.isfinite(err).all()), k
        worst[k] = (float((err * keep[k]).max()), bnd[k][0], float((err / bnd[k][1].clamp_min(1e-300))[keep[k]].max()) if bnd[k][1].max() > 0 else 0.0)
    print("roi_gn %s R=%d HW=%d C=%d relu=%d: " % (tag, c["R"], c["HW"], c["C"], c["relu"])
          + "  ".join("%s err %.3g (torch fp32 %.3g, %.2f of the bound)" % ((k,) + worst[k]) for k in worst))
    for k in ("y", "dx", "dga", "dbe"):
        err = (got[k].double().cpu() - c["ref"][k]).abs()
        assert bool((err <= bnd[k][1])[keep[k]].all()), (k, worst[k])


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", R64.SHAPES, ids=lambda s: "R%d_HW%d_C%d" % s[:3])
def test_against_float64(shape, kind, relu):
    dt = select(kind)
    check(R64.case(*shape, relu, False, None if kind == "fp32" else dt), dt, kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", R64.OFFCENTRE, ids=lambda s: "R%d_HW%d_C%d" % s[:3])
def test_off_centre_inputs(shape, kind):
    """mean 100, std 1: the centred statistics keep the variance's digits"""
    dt = select(kind)
    check(R64.case(*shape, True, True, None if kind == "fp32" else dt), dt, kind + " off-centre")


def test_padding_slots_stay_finite():
    """an all-zero ROI (ROI 1 of the 5-ROI cases): y = relu(beta), rstd = 1 / sqrt(eps), finite gradients"""
    select("fp32")
    c = R64.case(5, 49, 256, 32, True)
    got = run(c, torch.float32)
    assert torch.equal(got["y"][1].cpu(), torch.relu(c["be"]).expand(49, 256))
    assert bool((got["mean"][1] == 0).all()) and torch.allclose(got["rstd"][1].cpu(), torch.full((32,), R64.EPS ** -0.5))
    assert bool(torch.isfinite(got["dx"]).all())


@pytest.mark.parametrize("shape", [(2100, 4, 128, 32), (37, 49, 256, 32)], ids=lambda s: "R%d_HW%d_C%d" % s[:3])
def test_parameter_gradients_are_bit_identical_across_runs(shape):
    select("fp32")
    a, b = run(R64.case(*shape, True), torch.float32), run(R64.case(*shape, True), torch.float32)
    assert torch.equal(a["dga"], b["dga"]) and torch.equal(a["dbe"], b["dbe"]) and torch.equal(a["dx"], b["dx"])
    assert float(a["dga"].abs().max()) > 0


def test_parameter_gradients_accumulate():
    from ubteacher import hip
    select("fp32")
    c = R64.case(5, 4, 128, 32, True)
    got = run(c, torch.float32)
    x, dy, ga, be = c["x"].cuda(), c["dy"].cuda(), c["ga"].cuda(), c["be"].cuda()
    dga, dbe = torch.full_like(ga, 2.0), torch.full_like(be, -3.0)
    hip.groupnorm_roi_bwd(dy, x, got["mean"], got["rstd"], ga, be, dga, dbe, 32, True)
    assert torch.equal(dga, 2.0 + got["dga"]) and torch.equal(dbe, -3.0 + got["dbe"])


def test_argument_errors_and_empty_batch():
    from ubteacher import hip
    select("fp32")
    ga, be = torch.ones(128, device="cuda"), torch.zeros(128, device="cuda")
    with pytest.raises(RuntimeError, match="-1000"):       # (C / G) % 4 != 0
        hip.groupnorm_roi_fwd(torch.zeros(2, 4, 128, device="cuda"), ga, be, 64)
    with pytest.raises(RuntimeError, match="-1000"):       # HW 197
        hip.groupnorm_roi_fwd(torch.zeros(2, 197, 128, device="cuda"), ga, be, 32)
    x = torch.zeros(2, 4, 128, device="cuda")
    m = torch.zeros(2, 32, device="cuda")
    with pytest.raises(RuntimeError, match="-1000"):
        hip.groupnorm_roi_bwd(x, x, m, m, ga, be, torch.zeros_like(ga), torch.zeros_like(be), 64)
    with pytest.raises(RuntimeError, match="-1000"):
        xl = torch.zeros(2, 197, 128, device="cuda")
        hip.groupnorm_roi_bwd(xl, xl, m, m, ga, be, torch.zeros_like(ga), torch.zeros_like(be), 32)
    # R 0: OK, nothing launched, nothing accumulated
    e = torch.zeros(0, 49, 128, device="cuda")
    y, mean, rstd = hip.groupnorm_roi_fwd(e, ga, be, 32)
    assert tuple(y.shape) == (0, 49, 128) and tuple(mean.shape) == (0, 32)
    dga = torch.full_like(ga, 5.0)
    dx = hip.groupnorm_roi_bwd(e, e, mean, rstd, ga, be, dga, torch.zeros_like(be), 32)
    assert tuple(dx.shape) == (0, 49, 128) and bool((dga == 5.0).all())
