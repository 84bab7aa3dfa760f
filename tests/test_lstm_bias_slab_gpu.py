"""Bias-gradient slab of the LSTM backward pointwise kernel, and the in-place
recurrent addmm of the sequence backward.

Tolerances are derived, not tuned:
  * the reference for a bias gradient is the float64 column sum of the
    grad_gates the kernel itself wrote (bf16 / f32 values are exact in f64);
  * an f32 sum of n addends, in any order, is within n * 2^-24 * sum|x| of
    the exact sum — that is the atol of every f32 slab check, with no rtol;
  * where the sequence op rounds the result to bf16, 2^-8 * |ref| is added
    (round-to-nearest, 8 significant bits).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from nerrf_amd.ops import reference as ref  # noqa: E402

U32 = 2.0 ** -24
UBF16 = 2.0 ** -8


@pytest.fixture(autouse=True)
def _require_native(gpu_device):
    from nerrf_amd.ops.native import load_extension

    load_extension(required=True)


def _ext():
    from nerrf_amd.ops.native import load_extension

    return load_extension(required=True)


def _step_inputs(b, hd, dtype, dev, seed, masked):
    g = torch.Generator(device=dev).manual_seed(seed)

    def rn(*shape, scale=0.2):
        return (torch.randn(*shape, device=dev, generator=g) * scale).to(dtype)

    gacts = torch.sigmoid(torch.randn(b, 4 * hd, device=dev, generator=g)).to(dtype)
    mask = (
        (torch.rand(b, device=dev, generator=g) > 0.2).float()
        if masked else torch.empty(0, device=dev)
    )
    if masked:
        mask[b // 2] = 0.0  # small batches too have a masked row
    return dict(gh=rn(b, hd), gout=rn(b, hd), gc=rn(b, hd), gacts=gacts,
                c=rn(b, hd), mask=mask)


def _run_step(inp, accum, strided):
    """One kernel call.  Returns (grad_gates, grad_c_prev, grad_h_pass, used,
    sentinel_ok) — with `strided`, grad_gates is the SECOND 4H slab of a
    [B, 2*4H] buffer whose first slab must stay untouched."""
    b, hd = inp["c"].shape
    dev, dt = inp["c"].device, inp["c"].dtype
    if strided:
        buf = torch.full((b, 8 * hd), 7.0, device=dev, dtype=dt)
        gg = buf[:, 4 * hd:]
    else:
        buf = None
        gg = torch.empty(b, 4 * hd, device=dev, dtype=dt)
    gcp = torch.empty(b, hd, device=dev, dtype=dt)
    ghp = torch.empty(b, hd, device=dev, dtype=dt)
    used = _ext().lstm_pointwise_bwd(
        inp["gh"], inp["gout"], inp["gc"], inp["gacts"], inp["c"], inp["mask"],
        gg, gcp, ghp,
        accum if accum is not None else torch.empty(0, device=dev),
    )
    sentinel_ok = True if buf is None else bool((buf[:, :4 * hd] == 7.0).all())
    return gg, gcp, ghp, bool(used), sentinel_ok


def _assert_within(got64, ref64, bound64, what):
    err = (got64 - ref64).abs()
    worst = (err - bound64).max().item()
    print(f"{what}: max err {err.max().item():.3e}, "
          f"min bound {bound64.min().item():.3e}, max(err-bound) {worst:.3e}")
    assert bool((err <= bound64).all()), what


# (dtype, H, B, P, strided grad_gates, masked) — what each row covers:
STEP_CASES = [
    # partial last block; most slab rows must stay exactly 0
    pytest.param(torch.bfloat16, 256, 37, 64, False, True, id="bf16-B37-P64"),
    # many grid-stride iterations per thread, row tail
    pytest.param(torch.bfloat16, 256, 3001, 5, False, True, id="bf16-B3001-P5"),
    # P far above the grid; rows beyond the grid bitwise 0
    pytest.param(torch.bfloat16, 256, 8, 2048, False, True, id="bf16-B8-P2048"),
    # row stride 2048: the sum must cover only its own slab
    pytest.param(torch.bfloat16, 256, 130, 64, True, True, id="bf16-strided"),
    # no mask (the masked variant is every other row of this table)
    pytest.param(torch.bfloat16, 256, 130, 7, False, False, id="bf16-nomask"),
    # hv >= 64: no two lanes of a wave share a column group (no shuffle
    # round; 4, 2 and 1 thread groups per block)
    pytest.param(torch.bfloat16, 512, 37, 64, False, True, id="bf16-H512"),
    pytest.param(torch.bfloat16, 1024, 21, 64, False, True, id="bf16-H1024"),
    pytest.param(torch.bfloat16, 2048, 9, 3, False, True, id="bf16-H2048"),
    # f32, V=4, hv=16: two shuffle rounds inside a wave
    pytest.param(torch.float32, 64, 37, 64, False, True, id="f32-B37-P64"),
    pytest.param(torch.float32, 64, 3001, 5, False, True, id="f32-B3001-P5"),
    pytest.param(torch.float32, 64, 8, 2048, False, True, id="f32-B8-P2048"),
    pytest.param(torch.float32, 64, 130, 64, True, False, id="f32-strided-nomask"),
]


@pytest.mark.parametrize("dtype,hd,b,p,strided,masked", STEP_CASES)
def test_bias_slab_step(gpu_device, dtype, hd, b, p, strided, masked):
    inp = _step_inputs(b, hd, dtype, gpu_device, 100 + b + p, masked)
    gdim = 4 * hd
    vec = 8 if dtype == torch.bfloat16 else 4

    gg0, gcp0, ghp0, used0, ok0 = _run_step(inp, None, strided)
    assert not used0 and ok0

    slab = torch.zeros(p, gdim, device=gpu_device, dtype=torch.float32)
    gg, gcp, ghp, used, ok = _run_step(inp, slab, strided)
    assert used and ok
    # the accumulating kernel stores exactly what the plain one stores
    assert torch.equal(gg, gg0)
    assert torch.equal(gcp, gcp0)
    assert torch.equal(ghp, ghp0)

    gg64 = gg.double()
    ref64 = gg64.sum(0)
    bound = b * U32 * gg64.abs().sum(0)
    if masked:
        # masked rows store exact zeros and add 0 to the sum
        dead = inp["mask"] == 0
        assert bool(dead.any()) and bool((gg[dead] == 0).all())
    _assert_within(slab.double().sum(0), ref64, bound, "single call")

    # rows beyond the grid are never touched
    grid = min(p, max(1, -(-b * (hd // vec) // 256)))
    assert bool((slab[grid:] == 0).all())

    # accumulates across calls into one slab: 3n addends, 3x the magnitudes
    _run_step(inp, slab, strided)
    _run_step(inp, slab, strided)
    _assert_within(slab.double().sum(0), 3 * ref64, 3 * b * U32 * 3 * gg64.abs().sum(0),
                   "three calls")
    assert bool((slab[grid:] == 0).all())

    # no atomics: the same call into fresh slabs is bitwise reproducible
    s1 = torch.zeros(p, gdim, device=gpu_device, dtype=torch.float32)
    s2 = torch.zeros(p, gdim, device=gpu_device, dtype=torch.float32)
    _run_step(inp, s1, strided)
    _run_step(inp, s2, strided)
    assert torch.equal(s1, s2)


def test_bias_slab_unsupported_width_returns_false(gpu_device):
    """bf16 H=24: hv = 3 does not divide 256, so the fused path must refuse,
    leave the slab alone and still compute grad_gates."""
    b, hd = 50, 24
    inp = _step_inputs(b, hd, torch.bfloat16, gpu_device, 7, True)
    slab = torch.zeros(64, 4 * hd, device=gpu_device, dtype=torch.float32)
    gg, gcp, ghp, used, _ = _run_step(inp, slab, False)
    assert used is False
    assert bool((slab == 0).all())
    gg0, gcp0, ghp0, _, _ = _run_step(inp, None, False)
    assert torch.equal(gg, gg0) and torch.equal(gcp, gcp0) and torch.equal(ghp, ghp0)
    gg_ref, _, _ = ref.lstm_pointwise_bwd_ref(
        inp["gh"].float() + inp["gout"].float(), inp["gc"].float(),
        inp["gacts"].float(), inp["c"].float(), inp["mask"],
    )
    # the kernel evaluates the same f32 expression and rounds once to bf16
    # (2^-8 relative); 1e-4 relative covers the f32 evaluation differences
    # (device tanhf / fused multiply-adds, amplified by 1 - tanh^2 <= ~4x at
    # these magnitudes); 1e-6 absolute for values near zero
    assert torch.allclose(gg.float(), gg_ref, rtol=UBF16 + 1e-4, atol=1e-6)


# --------------------------------------------------------------------------
# sequence level
# --------------------------------------------------------------------------

def _seq_setup(t, b, hd, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    gd = 4 * hd

    def rn(*shape, scale):
        return (torch.randn(*shape, device=dev, generator=g) * scale).to(torch.bfloat16)

    lengths = torch.randint(1, t + 1, (b,), device=dev, generator=g)
    lengths[0] = 1  # at least one row of length 1
    lengths[1] = t
    mask = (torch.arange(t, device=dev)[:, None] < lengths[None, :]).float()
    return dict(
        xg2=rn(t, b, 2 * gd, scale=0.4), h0=rn(b, hd, scale=0.3),
        c0=rn(b, hd, scale=0.3), w_f=rn(gd, hd, scale=0.05),
        w_b=rn(gd, hd, scale=0.05), b_f=rn(gd, scale=0.5), b_b=rn(gd, scale=0.5),
        mask=mask, g_out=rn(t, b, 2 * hd, scale=1.0),
    )


def _leaf(x):
    return x.clone().requires_grad_(True)


def _run_bilayer2(s):
    from nerrf_amd.ops.lstm_seq import lstm_bilayer2

    p = {k: _leaf(s[k]) for k in ("xg2", "h0", "c0", "w_f", "b_f", "w_b", "b_b")}
    out = lstm_bilayer2(p["xg2"], p["h0"], p["c0"], p["w_f"], p["b_f"],
                        p["w_b"], p["b_b"], s["mask"])
    out.backward(s["g_out"])
    return {k: v.grad for k, v in p.items()}


def _run_single(s, reverse):
    from nerrf_amd.ops.lstm_seq import lstm_sequence

    hd = s["h0"].shape[1]
    gd = 4 * hd
    xg = s["xg2"][:, :, gd:] if reverse else s["xg2"][:, :, :gd]
    p = dict(xg=_leaf(xg.contiguous()), h0=_leaf(s["h0"]), c0=_leaf(s["c0"]),
             w=_leaf(s["w_b"] if reverse else s["w_f"]),
             b=_leaf(s["b_b"] if reverse else s["b_f"]))
    out = lstm_sequence(p["xg"], p["h0"], p["c0"], p["w"], p["b"], s["mask"],
                        reverse=reverse)
    g_out = s["g_out"][:, :, hd:] if reverse else s["g_out"][:, :, :hd]
    out.backward(g_out.contiguous())
    return {k: v.grad for k, v in p.items()}


def _check_bias(bias_grad, gg, what):
    """bias_grad [4H] (bf16) against the f64 column sum of gg [T, B, 4H]."""
    gg64 = gg.double().reshape(-1, gg.shape[-1])
    ref64 = gg64.sum(0)
    bound = gg64.shape[0] * U32 * gg64.abs().sum(0) + UBF16 * ref64.abs()
    _assert_within(bias_grad.double(), ref64, bound, what)


@pytest.mark.parametrize("t", [5, 1])
def test_bias_slab_bilayer2_matches_separate_reduction(gpu_device, monkeypatch, t):
    b, hd = 70, 256
    gd = 4 * hd
    s = _seq_setup(t, b, hd, gpu_device, 11 + t)
    monkeypatch.setenv("NERRF_FUSED_BIAS", "0")
    g0 = _run_bilayer2(s)
    monkeypatch.setenv("NERRF_FUSED_BIAS", "1")
    g1 = _run_bilayer2(s)

    assert torch.equal(g0["xg2"], g1["xg2"])
    for name, g in (("flag0", g0), ("flag1", g1)):
        _check_bias(g["b_f"], g["xg2"][:, :, :gd], f"{name} b_f T={t}")
        _check_bias(g["b_b"], g["xg2"][:, :, gd:], f"{name} b_b T={t}")
    # the tolerances of test_lstm_bilayer2_matches_bilayer
    for k in ("h0", "c0", "w_f", "w_b"):
        assert torch.allclose(g0[k].float(), g1[k].float(), atol=1e-5), k
    assert bool(g1["h0"].float().abs().max() > 0)


@pytest.mark.parametrize("reverse", [False, True])
def test_bias_slab_single_direction(gpu_device, monkeypatch, reverse):
    t, b, hd = 5, 70, 256
    s = _seq_setup(t, b, hd, gpu_device, 23)
    monkeypatch.setenv("NERRF_FUSED_BIAS", "0")
    g0 = _run_single(s, reverse)
    monkeypatch.setenv("NERRF_FUSED_BIAS", "1")
    g1 = _run_single(s, reverse)
    assert torch.equal(g0["xg"], g1["xg"])
    _check_bias(g0["b"], g0["xg"], f"flag0 reverse={reverse}")
    _check_bias(g1["b"], g1["xg"], f"flag1 reverse={reverse}")
    for k in ("h0", "c0", "w"):
        assert torch.allclose(g0[k].float(), g1[k].float(), atol=1e-5), k


def test_inplace_recurrent_addmm_matches_cpu_reference_f32(gpu_device):
    """Pins the grad_h / grad_h_pass ping-pong: an f32 run through the HIP
    kernels and the in-place addmm against the pure-PyTorch path on the CPU
    (tolerance of test_lstm_cell_bwd_fp32; a swapped buffer is off by the
    size of the gradient itself)."""
    from nerrf_amd.ops.lstm_seq import lstm_bilayer2

    t, b, hd = 4, 33, 64
    gd = 4 * hd
    g = torch.Generator().manual_seed(5)
    lengths = torch.randint(1, t + 1, (b,), generator=g)
    lengths[0] = 1
    mask = (torch.arange(t)[:, None] < lengths[None, :]).float()
    base = dict(
        xg2=torch.randn(t, b, 2 * gd, generator=g) * 0.4,
        h0=torch.randn(b, hd, generator=g) * 0.3,
        c0=torch.randn(b, hd, generator=g) * 0.3,
        w_f=torch.randn(gd, hd, generator=g) * 0.1,
        b_f=torch.randn(gd, generator=g) * 0.5,
        w_b=torch.randn(gd, hd, generator=g) * 0.1,
        b_b=torch.randn(gd, generator=g) * 0.5,
    )
    g_out = torch.randn(t, b, 2 * hd, generator=g)
    names = ("xg2", "h0", "c0", "w_f", "b_f", "w_b", "b_b")

    def run(dev):
        p = {k: base[k].to(dev).requires_grad_(True) for k in names}
        out = lstm_bilayer2(*(p[k] for k in names), mask.to(dev))
        out.backward(g_out.to(dev))
        return {k: v.grad.cpu() for k, v in p.items()}

    got, want = run(gpu_device), run(torch.device("cpu"))
    for k in names:
        assert torch.allclose(got[k], want[k], atol=1e-3, rtol=1e-3), k
