"""Row-count arguments of the LSTM pointwise kernels (prev_rows, in_rows, null
grad_h_pass) and the packed BiLSTM path through the HIP kernels.

Tolerances are the ones the project already uses for the same comparisons:
  * a kernel against itself with poisoned-but-unread rows: bitwise;
  * bias slab against the f64 column sum of the grad_gates the kernel
    stored: n * 2^-24 * sum|x| (test_lstm_bias_slab_gpu.py);
  * f32 HIP path against the CPU reference: atol = rtol = 1e-3
    (test_inplace_recurrent_addmm_matches_cpu_reference_f32);
  * bf16 packed against bf16 dense: atol = rtol = 3e-2, the project's bf16
    tolerance.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
NAN = float("nan")


@pytest.fixture(autouse=True)
def _require_native(gpu_device):
    from nerrf_amd.ops.native import load_extension

    load_extension(required=True)


def _ext():
    from nerrf_amd.ops.native import load_extension

    return load_extension(required=True)


def _rn(g, dev, dtype, *shape, scale=0.3):
    return (torch.randn(*shape, device=dev, generator=g) * scale).to(dtype)


def _rows(batch, width, odd, dev, dtype):
    """[batch, width] output target; `odd`: rows of a wider buffer whose row
    stride is no multiple of the vector width (-> scalar instantiation)."""
    if odd:
        return torch.zeros(batch, width + 1, device=dev, dtype=dtype)[:, :width]
    return torch.zeros(batch, width, device=dev, dtype=dtype)


# (dtype, H, odd row stride) -> bf16 V=8, f32 V=4, f32 scalar
KERNEL_CASES = [
    pytest.param(torch.bfloat16, 256, False, id="bf16-H256-vec8"),
    pytest.param(torch.float32, 64, False, id="f32-H64-vec4"),
    pytest.param(torch.float32, 64, True, id="f32-H64-scalar"),
]


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("dtype,hd,odd", KERNEL_CASES)
def test_fwd_prev_rows_never_reads_past_them(gpu_device, dtype, hd, odd, masked):
    dev, batch, prev = gpu_device, 300, 130
    g = torch.Generator(device=dev).manual_seed(7)
    hg = _rn(g, dev, dtype, batch, 4 * hd)
    xg = _rn(g, dev, dtype, batch, 4 * hd)
    bias = _rn(g, dev, dtype, 4 * hd)
    c_prev = _rn(g, dev, dtype, batch, hd)
    h_prev = _rn(g, dev, dtype, batch, hd)
    mask = (
        (torch.rand(batch, device=dev, generator=g) > 0.3).float()
        if masked else torch.empty(0, device=dev)
    )
    if masked:
        mask[prev + 5] = 0.0  # a masked row past the previous state

    def run(hg_, c_, h_, rows):
        h_out = _rows(batch, hd, odd, dev, dtype)
        c_out = torch.zeros(batch, hd, device=dev, dtype=dtype)
        gates = torch.zeros(batch, 4 * hd, device=dev, dtype=dtype)
        args = (hg_, xg, bias, c_, h_, mask, h_out, c_out, gates)
        if rows is None:
            _ext().lstm_pointwise_fwd(*args)  # the positional call of old
        else:
            _ext().lstm_pointwise_fwd(*args, rows)
        return h_out, c_out, gates

    poisoned = [t.clone() for t in (hg, c_prev, h_prev)]
    zeroed = [t.clone() for t in (hg, c_prev, h_prev)]
    for p, z in zip(poisoned, zeroed):
        p[prev:] = NAN
        z[prev:] = 0
    got = run(*poisoned, prev)
    want = run(*zeroed, None)
    for a, b, name in zip(got, want, ("h", "c", "gates")):
        assert bool(torch.isfinite(a).all()), name
        assert torch.equal(a, b), name
    # the previous state may also simply be that short
    short = run(hg[:prev], c_prev[:prev], h_prev[:prev], prev)
    for a, b in zip(short, want):
        assert torch.equal(a, b)
    # prev_rows = 0: no previous state at all
    z0 = run(torch.zeros_like(hg), torch.zeros_like(c_prev),
             torch.zeros_like(h_prev), None)
    n0 = run(hg[:0], c_prev[:0], h_prev[:0], 0)
    for a, b in zip(n0, z0):
        assert torch.equal(a, b)


@pytest.mark.parametrize("slab_on", [False, True], ids=["noslab", "slab"])
@pytest.mark.parametrize("dtype,hd,odd", KERNEL_CASES)
def test_bwd_in_rows_prev_rows_null_pass(gpu_device, dtype, hd, odd, slab_on):
    dev, batch, rin, prev = gpu_device, 300, 130, 90
    g = torch.Generator(device=dev).manual_seed(9)
    gh = _rn(g, dev, dtype, batch, hd)
    gout = _rn(g, dev, dtype, batch, hd)
    gc = _rn(g, dev, dtype, batch, hd)
    gacts = torch.sigmoid(torch.randn(batch, 4 * hd, device=dev, generator=g)).to(dtype)
    c_prev = _rn(g, dev, dtype, batch, hd)
    empty = torch.empty(0, device=dev)

    def run(gh_, gc_, c_, rows, null_pass):
        gg = _rows(batch, 4 * hd, odd, dev, dtype)
        gcp = torch.zeros(batch, hd, device=dev, dtype=dtype)
        ghp = (torch.empty(0, device=dev, dtype=dtype) if null_pass
               else torch.full((batch, hd), 5.0, device=dev, dtype=dtype))
        slab = (torch.zeros(64, 4 * hd, device=dev, dtype=torch.float32)
                if slab_on else empty)
        args = (gh_, gout, gc_, gacts, c_, empty, gg, gcp, ghp, slab)
        used = _ext().lstm_pointwise_bwd(*args, *rows)
        return gg, gcp, ghp, slab, bool(used)

    poisoned = [t.clone() for t in (gh, gc, c_prev)]
    zeroed = [t.clone() for t in (gh, gc, c_prev)]
    for (p, z), n in zip(zip(poisoned, zeroed), (rin, rin, prev)):
        p[n:] = NAN
        z[n:] = 0
    gg, gcp, _, slab, used = run(*poisoned, (rin, prev), True)
    gg0, gcp0, ghp0, slab0, used0 = run(*zeroed, (), False)
    assert bool(torch.isfinite(gg).all()) and bool(torch.isfinite(gcp).all())
    assert torch.equal(gg, gg0) and torch.equal(gcp, gcp0)
    assert bool((ghp0 == 0).all())  # what the null pointer leaves unwritten
    assert used == used0 == (slab_on and not odd)
    if used:
        assert torch.equal(slab, slab0)
        gg64 = gg.double()
        err = (slab.double().sum(0) - gg64.sum(0)).abs()
        bound = batch * U32 * gg64.abs().sum(0)
        print(f"slab max err {err.max().item():.3e}, min bound {bound.min().item():.3e}")
        assert bool((err <= bound).all())
    elif slab_on:
        assert bool((slab == 0).all())
    # the incoming state may also simply be that short
    short = run(gh[:rin], gc[:rin], c_prev[:prev], (rin, prev), True)
    assert torch.equal(short[0], gg0) and torch.equal(short[1], gcp0)


def test_zero_row_calls_launch_nothing(gpu_device):
    dev, hd = gpu_device, 256
    bf = dict(device=dev, dtype=torch.bfloat16)
    e2 = lambda w: torch.empty(0, w, **bf)  # noqa: E731
    empty = torch.empty(0, device=dev)
    _ext().lstm_pointwise_fwd(e2(4 * hd), e2(4 * hd), torch.zeros(4 * hd, **bf),
                              e2(hd), e2(hd), empty, e2(hd), e2(hd), e2(4 * hd))
    used = _ext().lstm_pointwise_bwd(e2(hd), e2(hd), e2(hd), e2(4 * hd), e2(hd),
                                     empty, e2(4 * hd), e2(hd), e2(hd), empty)
    assert not used
    _ext().rec_gemm_fwd(e2(hd), torch.zeros(4 * hd, hd, **bf), e2(4 * hd))
    torch.cuda.synchronize()  # a grid of 0 would have raised a launch error


def test_vector_path_rejects_misaligned_base(gpu_device):
    """A row slice of a packed buffer starts at a row offset: the bindings
    check the base address, not only the strides."""
    dev, batch, hd = gpu_device, 4, 64
    f32 = dict(device=dev, dtype=torch.float32)
    flat = torch.zeros(batch * hd + 1, **f32)
    c_off = flat[1:].view(batch, hd)  # 4-byte aligned only
    z = lambda w: torch.zeros(batch, w, **f32)  # noqa: E731
    with pytest.raises(RuntimeError, match="16-byte"):
        _ext().lstm_pointwise_fwd(z(4 * hd), z(4 * hd), torch.zeros(4 * hd, **f32),
                                  c_off, z(hd), torch.empty(0, device=dev),
                                  z(hd), z(hd), z(4 * hd))


def _mixed_lengths(b, t, seed):
    g = torch.Generator().manual_seed(seed)
    ln = torch.randint(1, t + 1, (b,), generator=g)
    ln[0], ln[1], ln[2] = 1, t, 1
    return ln


def test_bilayer2_packed_matches_cpu_reference_f32(gpu_device):
    from nerrf_amd.ops.lstm_seq import build_seq_plan, lstm_bilayer2_packed

    t, b, hd = 6, 33, 64
    gd = 4 * hd
    lengths = _mixed_lengths(b, t, 5)
    n = int(lengths.sum())
    g = torch.Generator().manual_seed(6)
    base = dict(
        xg2p=torch.randn(n, 2 * gd, generator=g) * 0.4,
        w_f=torch.randn(gd, hd, generator=g) * 0.1,
        b_f=torch.randn(gd, generator=g) * 0.5,
        w_b=torch.randn(gd, hd, generator=g) * 0.1,
        b_b=torch.randn(gd, generator=g) * 0.5,
    )
    g_out = torch.randn(n, 2 * hd, generator=g)
    names = ("xg2p", "w_f", "b_f", "w_b", "b_b")

    def run(dev):
        plan = build_seq_plan(lengths.numpy(), t, dev)
        assert plan.n_rows == n
        p = {k: base[k].to(dev).requires_grad_(True) for k in names}
        out = lstm_bilayer2_packed(p["xg2p"], plan, p["w_f"], p["b_f"],
                                   p["w_b"], p["b_b"])
        out.backward(g_out.to(dev))
        return out.detach().cpu(), {k: v.grad.cpu() for k, v in p.items()}

    got_o, got = run(gpu_device)
    want_o, want = run(torch.device("cpu"))
    assert torch.allclose(got_o, want_o, atol=1e-3, rtol=1e-3)
    for k in names:
        err = (got[k] - want[k]).abs().max().item()
        assert torch.allclose(got[k], want[k], atol=1e-3, rtol=1e-3), (k, err)
        assert bool(want[k].abs().max() > 0), k


def test_packed_forward_is_bitwise_the_dense_forward_bf16(gpu_device):
    """Same kernels per row as the dense training path (rec_gemm.hip on every
    step, the pointwise kernel with mask = 1 is the unmasked arithmetic), and
    both compute each row independently of how many rows the launch has: the
    live rows of the dense output and the packed output are the same bits."""
    from nerrf_amd.ops.lstm_seq import build_seq_plan, lstm_bilayer2, lstm_bilayer2_packed

    t, b, hd = 6, 150, 256
    gd = 4 * hd
    dev, dt = gpu_device, torch.bfloat16
    lengths = _mixed_lengths(b, t, 12)
    plan = build_seq_plan(lengths.numpy(), t, dev)
    g = torch.Generator(device=dev).manual_seed(4)
    xg2 = _rn(g, dev, dt, t, b, 2 * gd, scale=0.4).requires_grad_(True)
    w = [_rn(g, dev, dt, gd, hd, scale=0.05), _rn(g, dev, dt, gd, scale=0.5),
         _rn(g, dev, dt, gd, hd, scale=0.05), _rn(g, dev, dt, gd, scale=0.5)]
    mask = (torch.arange(t)[:, None] < lengths[None, :]).float().to(dev)
    zeros = torch.zeros(b, hd, device=dev, dtype=dt)
    dense = lstm_bilayer2(xg2, zeros, zeros, *w, mask).detach()
    # packed row (t, r) is time-major row t * b + perm[r]
    rows = torch.cat([
        ti * b + torch.from_numpy(plan.perm[:n]) for ti, n in enumerate(plan.batch_sizes)
    ]).to(dev)
    xg2p = xg2.detach().reshape(t * b, 2 * gd).index_select(0, rows).requires_grad_(True)
    packed = lstm_bilayer2_packed(xg2p, plan, *w).detach()
    assert torch.equal(packed, dense.reshape(t * b, 2 * hd).index_select(0, rows))


def _model_lengths():
    # n_t = 300, 261, 220, 187, 137, 97, 38, 1: one step with a single live
    # row, no slab boundary on a multiple of 128
    counts = {8: 1, 7: 37, 6: 59, 5: 40, 4: 50, 3: 33, 2: 41, 1: 39}
    ln = torch.tensor([k for k, c in counts.items() for _ in range(c)])
    return ln[torch.randperm(ln.numel(), generator=torch.Generator().manual_seed(2))]


@pytest.mark.parametrize(
    "rec_gemm,min_rows",
    [("0", None), ("1", None), ("1", 128)],
    ids=["hipblaslt", "rec_gemm-every-step", "rec_gemm-from-128-rows"],
)
def test_packed_model_matches_dense_bf16(gpu_device, monkeypatch, rec_gemm, min_rows):
    from nerrf_amd.models.lstm import BiLSTMDetector, LSTMConfig
    from nerrf_amd.ops import lstm_seq

    monkeypatch.setenv("NERRF_REC_GEMM", rec_gemm)
    if min_rows is not None:  # steps of 97, 38 and 1 rows then go to hipBLASLt
        monkeypatch.setattr(lstm_seq, "_REC_GEMM_MIN_ROWS", min_rows)
    b, t = 300, 8
    lengths = _model_lengths().to(gpu_device)
    plan = lstm_seq.build_seq_plan(lengths, t, gpu_device)
    assert plan.batch_sizes == [300, 261, 220, 187, 137, 97, 38, 1]
    assert all(o % 128 for o in plan.offsets[1:])
    torch.manual_seed(0)
    model = BiLSTMDetector(LSTMConfig(in_dim=16, hidden=256, layers=2)).to(
        device=gpu_device, dtype=torch.bfloat16)
    g = torch.Generator().manual_seed(1)
    feats = torch.randn(b, t, 16, generator=g).to(device=gpu_device, dtype=torch.bfloat16)
    w = torch.randn(b, generator=g).to(device=gpu_device, dtype=torch.bfloat16)

    def run(packed):
        monkeypatch.setenv("NERRF_LSTM_PACKED", "1" if packed else "0")
        model.zero_grad(set_to_none=True)
        logits = model(feats, lengths)
        (logits * w).sum().backward()
        return logits.detach().float(), {
            k: p.grad.float().clone() for k, p in model.named_parameters()}

    want, want_g = run(False)
    got, got_g = run(True)
    assert torch.allclose(got, want, atol=3e-2, rtol=3e-2)
    for k in want_g:
        err = (got_g[k] - want_g[k]).abs().max().item()
        assert torch.allclose(got_g[k], want_g[k], atol=3e-2, rtol=3e-2), (k, err)
        assert bool(want_g[k].abs().max() > 0), k


def test_packed_op_with_plan_never_syncs(gpu_device):
    from nerrf_amd.ops.lstm_seq import build_seq_plan, lstm_bilayer2_packed

    t, b, hd = 5, 70, 256
    gd = 4 * hd
    dev, dt = gpu_device, torch.bfloat16
    lengths = _mixed_lengths(b, t, 8)
    plan = build_seq_plan(lengths.numpy(), t, dev)
    g = torch.Generator(device=dev).manual_seed(3)
    p = [
        _rn(g, dev, dt, plan.n_rows, 2 * gd, scale=0.4), _rn(g, dev, dt, gd, hd, scale=0.05),
        _rn(g, dev, dt, gd, scale=0.5), _rn(g, dev, dt, gd, hd, scale=0.05),
        _rn(g, dev, dt, gd, scale=0.5),
    ]
    for x in p:
        x.requires_grad_(True)
    g_out = _rn(g, dev, dt, plan.n_rows, 2 * hd, scale=1.0)
    # first calls may initialise the GEMM library; that is not the op's doing
    lstm_bilayer2_packed(p[0], plan, *p[1:]).backward(g_out)
    torch.cuda.synchronize()
    prev_mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = lstm_bilayer2_packed(p[0], plan, *p[1:])
        out.backward(g_out)
    finally:
        torch.cuda.set_sync_debug_mode(prev_mode)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(x.grad.float()).all()) for x in p)
