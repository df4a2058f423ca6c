"""kubeflow_rm_amd.optim.AdamW: torch.optim.AdamW's update; bf16 CUDA parameters on the multi-tensor
HIP kernel (kernels/adamw_bf16.hip), everything else on torch's functional AdamW."""
import math

import pytest
import torch

from kubeflow_rm_amd.optim import AdamW


def test_cpu_fp32_matches_torch_adamw():
    torch.manual_seed(0)
    a, b = torch.nn.Linear(16, 8), torch.nn.Linear(16, 8)
    b.load_state_dict(a.state_dict())
    oa = AdamW(a.parameters(), lr=1e-2, weight_decay=0.1)
    ob = torch.optim.AdamW(b.parameters(), lr=1e-2, weight_decay=0.1)
    for _ in range(4):
        x = torch.randn(4, 16)
        for m, o in ((a, oa), (b, ob)):
            o.zero_grad()
            m(x).pow(2).sum().backward()
            o.step()
    for pa, pb in zip(a.parameters(), b.parameters()):
        assert torch.equal(pa, pb)


def test_rejects_bad_hyperparameters():
    with pytest.raises(ValueError):
        AdamW([torch.zeros(2, requires_grad=True)], lr=-1.0)
    with pytest.raises(ValueError):
        AdamW([torch.zeros(2, requires_grad=True)], betas=(1.0, 0.9))


@pytest.mark.gpu
def test_bf16_cuda_kernel_matches_reference():
    """Odd sizes (tails past the 8-element vectors, several chunks), a parameter without a gradient,
    re-allocated gradients: every step within two bf16 ulps of the same update emulated in fp32 with
    the kernel's rounding points (m, v, p rounded to bf16 once per step; fp32 operation order can flip
    a rounding). The emulation restarts from the kernel's state each step, so a flipped rounding is not
    carried. lr = 5e-2 makes a wrong update (no bias correction, wrong decay) far above the tolerance."""
    from kubeflow_rm_amd import ops
    assert ops.available()
    g0 = torch.Generator(device="cuda").manual_seed(0)
    shapes = [(1000, 37), (3,), (65536 * 2 + 5,), (256, 256)]
    ps = [torch.nn.Parameter((torch.rand(s, generator=g0, device="cuda") * 2 - 1).to(torch.bfloat16)) for s in shapes]
    idle = torch.nn.Parameter(torch.ones(8, device="cuda", dtype=torch.bfloat16))
    lr, b1, b2, eps, wd = 5e-2, 0.9, 0.95, 1e-8, 0.1
    opt = AdamW(ps + [idle], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    ref = [p.detach().clone() for p in ps]
    mr = [torch.zeros_like(p) for p in ps]
    vr = [torch.zeros_like(p) for p in ps]
    for t in range(1, 5):
        grads = [(torch.rand(p.shape, generator=g0, device="cuda") * 2 - 1).to(torch.bfloat16) for p in ps]
        for p, g in zip(ps, grads):
            p.grad = g.clone()
        opt.step()
        ss, ib = lr / (1 - b1 ** t), 1 / math.sqrt(1 - b2 ** t)
        for i, g in enumerate(grads):
            gf = g.float()
            m = b1 * mr[i].float() + (1 - b1) * gf
            v = b2 * vr[i].float() + (1 - b2) * gf * gf
            ref[i] = (ref[i].float() * (1 - lr * wd) - ss * m / (v.sqrt() * ib + eps)).to(torch.bfloat16)
            mr[i], vr[i] = m.to(torch.bfloat16), v.to(torch.bfloat16)
        torch.cuda.synchronize()
        for i, p in enumerate(ps):
            d = (p.detach().float() - ref[i].float()).abs()
            ulp = ref[i].float().abs().clamp(min=1e-6) * 2 ** -6  # two ulps
            assert bool((d <= ulp + 1e-6).all()), (t, i, d.max().item())
            assert torch.equal(opt.state[p]["exp_avg"].float().sub(mr[i].float()).abs().le(
                mr[i].float().abs() * 2 ** -6 + 1e-7).all(), torch.tensor(True, device="cuda"))
            dv = (opt.state[p]["exp_avg_sq"].float() - vr[i].float()).abs()
            assert bool((dv <= vr[i].float().abs() * 2 ** -6 + 1e-9).all()), (t, i, dv.max().item())
            # re-sync the emulation to the kernel's state: each step is checked on its own rounding
            ref[i] = p.detach().clone()
            mr[i] = opt.state[p]["exp_avg"].clone()
            vr[i] = opt.state[p]["exp_avg_sq"].clone()
    assert torch.equal(idle.detach(), torch.ones_like(idle))


def test_tensor_step_from_a_torch_state_becomes_an_int():
    """a state loaded from torch.optim.AdamW carries ``step`` as a tensor; it is normalised
    to an int, so launches group (and pointer tables cache) by value, not by tensor identity."""
    torch.manual_seed(0)
    m = torch.nn.Linear(4, 2)
    src = torch.optim.AdamW(m.parameters(), lr=1e-2)
    m(torch.randn(3, 4)).sum().backward()
    src.step()
    opt = AdamW(m.parameters(), lr=1e-2)
    opt.load_state_dict(src.state_dict())
    assert all(torch.is_tensor(opt.state[p]["step"]) for p in m.parameters())
    m(torch.randn(3, 4)).sum().backward()
    opt.step()
    assert all(opt.state[p]["step"] == 2 and isinstance(opt.state[p]["step"], int) for p in m.parameters())


@pytest.mark.gpu
def test_bf16_moments_track_an_unsynced_emulation_over_20_steps():
    """without re-syncing, the kernel's p / exp_avg / exp_avg_sq after 20 steps stay
    within bf16 rounding noise of the fp32 emulation (slow drift in v would show here), and one
    state-loaded parameter group keeps ONE cached pointer table."""
    g0 = torch.Generator(device="cuda").manual_seed(1)
    shapes = [(513, 129), (70_001,)]
    ps = [torch.nn.Parameter((torch.rand(s, generator=g0, device="cuda") * 2 - 1).to(torch.bfloat16)) for s in shapes]
    lr, b1, b2, eps, wd = 1e-2, 0.9, 0.95, 1e-8, 0.1
    opt = AdamW(ps, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    ref = [p.detach().float().clone() for p in ps]
    mr = [torch.zeros_like(r) for r in ref]
    vr = [torch.zeros_like(r) for r in ref]
    for t in range(1, 21):
        grads = [(torch.randn(p.shape, generator=g0, device="cuda") * 0.1).to(torch.bfloat16) for p in ps]
        for p, g in zip(ps, grads):
            p.grad = g.clone()
        opt.step()
        ss, ib = lr / (1 - b1 ** t), 1 / math.sqrt(1 - b2 ** t)
        for i, g in enumerate(grads):
            gf = g.float()
            mr[i] = b1 * mr[i] + (1 - b1) * gf
            vr[i] = b2 * vr[i] + (1 - b2) * gf * gf
            ref[i] = ref[i] * (1 - lr * wd) - ss * mr[i] / (vr[i].sqrt() * ib + eps)
    torch.cuda.synchronize()

    def rel(a, b):
        return ((a.float() - b).norm() / b.norm()).item()
    for i, p in enumerate(ps):
        assert rel(opt.state[p]["exp_avg"], mr[i]) < 1e-2, i
        assert rel(opt.state[p]["exp_avg_sq"], vr[i]) < 1e-2, i
        assert rel(p.detach(), ref[i]) < 1e-2, i
    assert len(opt._tables) == 1


# ---- the kernel's launch paths, chunk edges and pointer table, step by step ---------------------------
# Same emulation and the same two-ulp bounds as test_bf16_cuda_kernel_matches_reference: fp32 with the
# kernel's rounding points (m, v, p to bf16 once per step), restarted from the kernel's state each step.
DEV = "cuda"
CHUNK = 16384  # kfamd_adamw_chunk(): elements per block
SENTINEL = 0x7FA5  # a bf16 NaN: memory next to a tensor is compared by bits
HP = dict(lr=5e-2, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.1)


def _sync():
    torch.cuda.synchronize()


def _bits(t):
    return t.detach().contiguous().view(torch.int16).cpu()


def _rand(n, gen):
    return (torch.rand(n, generator=gen) * 2 - 1).to(torch.bfloat16).to(DEV)


def _sentinel_buffer(n):
    flat = torch.empty(n, dtype=torch.bfloat16, device=DEV)
    flat.view(torch.int16).fill_(SENTINEL)
    assert flat.data_ptr() % 16 == 0
    return flat


def _views(ns, gap=16):
    """One sentinel-filled flat buffer and the [start, end) of a view per n, each 1 element (2 B) past the
    16-B grid with at least ``gap`` sentinel elements on both sides."""
    spans, cur = [], gap
    for n in ns:
        spans.append((cur + 1, cur + 1 + n))
        cur = -(-(cur + 1 + n + gap) // 8) * 8
    return _sentinel_buffer(cur), spans


def _outside(flat, spans):
    keep = torch.ones(flat.numel(), dtype=torch.bool)
    for a, b in spans:
        keep[a:b] = False
    return _bits(flat)[keep]


def _emulate(p, g, m, v, t, lr, betas, eps, weight_decay):
    (b1, b2), wd = betas, weight_decay
    ss, ib = lr / (1 - b1 ** t), 1 / math.sqrt(1 - b2 ** t)
    gf = g.float()
    mf = b1 * m.float() + (1 - b1) * gf
    vf = b2 * v.float() + (1 - b2) * gf * gf
    pn = (p.float() * (1 - lr * wd) - ss * mf / (vf.sqrt() * ib + eps)).to(torch.bfloat16)
    return pn, mf.to(torch.bfloat16), vf.to(torch.bfloat16)


def _step_and_check(opt, ps, t, hp, tag):
    """opt.step() with the gradients the parameters hold; every p / exp_avg / exp_avg_sq element within the
    bounds of the emulated step from the state before it, and every gradient left bit-identical."""
    before = []
    for p in ps:
        st = opt.state[p] if p in opt.state else {}
        before.append((p.detach().clone(), p.grad.clone(),
                       st["exp_avg"].clone() if st else torch.zeros_like(p),
                       st["exp_avg_sq"].clone() if st else torch.zeros_like(p)))
    opt.step()
    _sync()
    for i, (p, (p0, g0, m0, v0)) in enumerate(zip(ps, before)):
        pr, mr, vr = (x.float() for x in _emulate(p0, g0, m0, v0, t, **hp))
        assert torch.equal(_bits(p.grad), _bits(g0)), (tag, t, i, "the gradient was written")
        assert opt.state[p]["step"] == t
        d = (p.detach().float() - pr).abs()
        assert bool((d <= pr.abs().clamp(min=1e-6) * 2 ** -6 + 1e-6).all()), (tag, t, i, d.max().item())
        dm = (opt.state[p]["exp_avg"].float() - mr).abs()
        assert bool((dm <= mr.abs() * 2 ** -6 + 1e-7).all()), (tag, t, i, dm.max().item())
        dv = (opt.state[p]["exp_avg_sq"].float() - vr).abs()
        assert bool((dv <= vr.abs() * 2 ** -6 + 1e-9).all()), (tag, t, i, dv.max().item())


def _one_table(opt, ps):
    """The single cached pointer table, which lists every one of ``ps``: all of them took the HIP kernel."""
    assert len(opt._tables) == 1
    (cached,) = opt._tables.values()
    assert [row[0] for row in cached[0]] == [p.data_ptr() for p in ps]
    assert [row[1] for row in cached[0]] == [p.grad.data_ptr() for p in ps]
    return cached


@pytest.mark.gpu
def test_bf16_kernel_scalar_path_views_off_the_16_byte_grid():
    """The kernel's all-scalar branch: parameters that are contiguous views 2 B past the 16-B grid of one flat
    buffer (sizes around one chunk), and an aligned parameter whose gradient alone is such a view. Three
    steps; the flat buffers' sentinels on both sides of every view keep their bits."""
    gen = torch.Generator().manual_seed(2)
    ns = [3, 8, CHUNK - 1, CHUNK, CHUNK + 1]
    flat, spans = _views(ns)
    ps = []
    for a, b in spans:
        flat[a:b].copy_(_rand(b - a, gen))
        ps.append(torch.nn.Parameter(flat[a:b]))
        assert ps[-1].data_ptr() == flat.data_ptr() + 2 * a and ps[-1].data_ptr() % 16 == 2
    ng = 4099
    gflat, gspans = _views([ng])
    ps.append(torch.nn.Parameter(_rand(ng, gen)))
    assert ps[-1].data_ptr() % 16 == 0
    opt = AdamW(ps, **HP)
    for t in range(1, 4):
        for p in ps[:-1]:
            p.grad = _rand(p.numel(), gen)
        gflat[gspans[0][0]:gspans[0][1]].copy_(_rand(ng, gen))
        ps[-1].grad = gflat[gspans[0][0]:gspans[0][1]]
        assert ps[-1].grad.data_ptr() % 16 == 2
        _step_and_check(opt, ps, t, HP, "scalar")
        _one_table(opt, ps)
        assert bool((_outside(flat, spans) == SENTINEL).all()), (t, "memory next to a parameter view was written")
        assert bool((_outside(gflat, gspans) == SENTINEL).all()), (t, "memory next to the gradient view was written")
    for p, (a, b) in zip(ps, spans):
        assert torch.equal(_bits(p), _bits(flat[a:b]))  # the views are the buffer


@pytest.mark.gpu
def test_bf16_kernel_chunk_edges_across_tensors_and_an_empty_parameter():
    """Fresh (aligned) tensors whose sizes sit on and around the 16384-element chunk, in ONE launch, so the
    chunk-owner map changes tensor at chunk edges; an empty parameter with a gradient in the middle takes
    no chunk and shifts nobody's."""
    gen = torch.Generator().manual_seed(3)
    ns = [8, CHUNK - 8, CHUNK, 0, CHUNK + 8, CHUNK + 1, 2 * CHUNK]
    ps = [torch.nn.Parameter(_rand(n, gen)) for n in ns]
    opt = AdamW(ps, **HP)
    for t in range(1, 3):
        for p in ps:
            p.grad = _rand(p.numel(), gen)
        _step_and_check(opt, ps, t, HP, "chunks")
        cached = _one_table(opt, ps)
        assert cached[3] == sum(-(-n // CHUNK) for n in ns) == 9  # chunks in the launch
    assert opt.state[ps[3]]["step"] == 2 and opt.state[ps[3]]["exp_avg"].numel() == 0


@pytest.mark.gpu
def test_bf16_only_empty_parameters_is_a_no_op():
    p = torch.nn.Parameter(torch.empty(0, dtype=torch.bfloat16, device=DEV))
    p.grad = torch.empty(0, dtype=torch.bfloat16, device=DEV)
    opt = AdamW([p], **HP)
    opt.step()
    _sync()
    assert opt.state[p]["step"] == 1 and not opt._tables


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["vector", "scalar"])
def test_bf16_kernel_zero_gradients_only_decay(path):
    """Where g == 0 on step 1, m and v stay +0 by bits and the update is 0 / eps = 0: p is exactly
    bf16(p * (1 - lr wd)). lr wd = 2^-5, so the decay factor is the same fp32 number however it is formed."""
    hp = dict(HP, lr=0.0625, weight_decay=0.5)
    gen = torch.Generator().manual_seed(4)
    n = CHUNK + 8 + 5
    if path == "vector":
        flat, p = None, torch.nn.Parameter(_rand(n, gen))
    else:
        flat, spans = _views([n])
        flat[spans[0][0]:spans[0][1]].copy_(_rand(n, gen))
        p = torch.nn.Parameter(flat[spans[0][0]:spans[0][1]])
    assert p.data_ptr() % 16 == (0 if path == "vector" else 2)
    p0 = p.detach().clone()
    g = _rand(n, gen)
    zero = torch.arange(n, device=DEV) % 2 == 0
    g[zero] = 0.0
    assert bool((g[~zero] != 0).any())
    p.grad = g
    opt = AdamW([p], **hp)
    _step_and_check(opt, [p], 1, hp, "zeros")
    _one_table(opt, [p])
    want = (p0.float() * (1 - hp["lr"] * hp["weight_decay"])).to(torch.bfloat16)
    assert torch.equal(_bits(p)[zero.cpu()], _bits(want)[zero.cpu()])
    assert bool((_bits(opt.state[p]["exp_avg"])[zero.cpu()] == 0).all())
    assert bool((_bits(opt.state[p]["exp_avg_sq"])[zero.cpu()] == 0).all())
    if flat is not None:
        assert bool((_outside(flat, spans) == SENTINEL).all())


@pytest.mark.gpu
def test_bf16_a_changed_lr_takes_effect_through_the_cached_table():
    """A scheduler writes group["lr"]; the pointers did not change, so the cached table is reused as it is, and
    the step must use the new lr (a tenth: the old one would miss the bound by far)."""
    gen = torch.Generator().manual_seed(5)
    ps = [torch.nn.Parameter(_rand(n, gen)) for n in (1000, CHUNK + 11)]
    for p in ps:
        p.grad = _rand(p.numel(), gen)
    opt = AdamW(ps, **HP)
    _step_and_check(opt, ps, 1, HP, "lr")
    cached = _one_table(opt, ps)
    hp = dict(HP, lr=HP["lr"] / 10)
    opt.param_groups[0]["lr"] = hp["lr"]
    for p in ps:
        p.grad.copy_(_rand(p.numel(), gen))  # new values at the same address
    _step_and_check(opt, ps, 2, hp, "lr")
    assert _one_table(opt, ps) is cached


@pytest.mark.gpu
def test_bf16_a_gradient_at_a_new_address_rebuilds_the_table():
    gen = torch.Generator().manual_seed(6)
    ps = [torch.nn.Parameter(_rand(n, gen)) for n in (1000, CHUNK + 11)]
    for p in ps:
        p.grad = _rand(p.numel(), gen)
    opt = AdamW(ps, **HP)
    _step_and_check(opt, ps, 1, HP, "regrad")
    cached = _one_table(opt, ps)
    old = ps[1].grad  # kept alive, so the new gradient cannot land on its address
    ps[1].grad = _rand(ps[1].numel(), gen)
    assert ps[1].grad.data_ptr() != old.data_ptr()
    old.fill_(100.0)  # a step through the stale pointer would be far off
    _step_and_check(opt, ps, 2, HP, "regrad")
    assert _one_table(opt, ps) is not cached
    assert bool((old == 100.0).all())
