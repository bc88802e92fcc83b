"""Adam / AdamW and gradient clipping (csrc/kernels/adam.hip) against a plain
fp64 Adam step: every option the optimizer forwards, every code path of the
flat kernel (vector body, scalar tail, unaligned fallback, grid-stride trip,
device scalars) and the Adam folded into the fused step's reduction.

The kernel forms ``1 - beta`` in fp32 from the fp32 beta, so the reference
rounds its scalars to fp32 first; with un-rounded scalars the same reference
is ``torch.optim.Adam`` in fp64 (checked on the CPU, below).

Every test here needs the GPU (``@gpu``) except that CPU check, which has to
run in the ``-m "not gpu"`` suite and therefore keeps this file from using a
module-level mark.  Each comparison prints its worst error as a fraction of
its tolerance (``RATIO <quantity> <value>``; run with ``-s`` to see them).
"""
import copy
import math

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu

HYPER = [(1e-2, 0.9, 0.999, 1e-8), (2.5e-3, 0.8, 0.95, 1e-6)]
# (weight_decay, decoupled, maximize, amsgrad, grad_scale)
OPTIONS = [
    (0.0, False, False, False, 1.0),
    (1e-2, False, False, False, 1.0),
    (1e-2, True, False, False, 0.125),
    (0.0, False, True, False, 1.0),
    (1e-2, False, True, True, 1.0),
    (1e-2, True, False, True, 0.5),
    (0.1, False, False, True, 1.0 / 3.0),
]


def _mod():
    from pytorch_distributed_rnn_amd import _ext
    return _ext.require()


def _f32(x):
    return float(np.float32(x))


def adam_ref(p, g, m, v, vmax, step, lr, b1, b2, eps, wd=0.0, decoupled=False, maximize=False,
             grad_scale=1.0, round_scalars=True):
    """One Adam step on fp64 tensors, in place (``vmax`` None: no amsgrad).
    The bias corrections come from the double betas; with ``round_scalars``
    they and every other scalar are rounded to fp32 as the native launch does."""
    r = _f32 if round_scalars else float
    bc1 = r(1.0 - b1 ** step)
    bc2_sqrt = r(math.sqrt(1.0 - b2 ** step))
    lr, b1, b2, eps, wd, grad_scale = r(lr), r(b1), r(b2), r(eps), r(wd), r(grad_scale)
    g = g * grad_scale
    if maximize:
        g = -g
    if wd != 0.0:
        if decoupled:
            p.mul_(1.0 - lr * wd)
        else:
            g = g + wd * p
    m.add_((1.0 - b1) * (g - m))
    v.mul_(b2).add_((1.0 - b2) * g * g)
    vv = v
    if vmax is not None:
        torch.maximum(vmax, v, out=vmax)
        vv = vmax
    denom = vv.sqrt() / bc2_sqrt + eps
    p.sub_((lr / bc1) * (m / denom))


def _ratio(name, got, ref, rtol, atol):
    """Worst |got - ref| / (atol + rtol |ref|), printed; <= 1 passes."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape
    if ref.numel() == 0:
        return 0.0
    assert torch.isfinite(got).all(), f"{name}: non-finite values"
    r = ((got - ref).abs() / (atol + rtol * ref.abs())).max().item()
    print(f"RATIO {name} {r:.4f}")
    return r


def _check_p(got, ref, what=""):
    r = _ratio("adam.p", got, ref, 1e-5, 1e-6)
    assert r <= 1.0, f"parameters{what}: {r:.3f} x (rtol 1e-5, atol 1e-6)"


def _check_moment(name, got, ref, what=""):
    atol = 1e-7 * ref.abs().max().item()
    r = _ratio(f"adam.{name}", got, ref, 1e-5, max(atol, 1e-300))
    assert r <= 1.0, f"{name}{what}: {r:.3f} x (rtol 1e-5, atol 1e-7 max|ref|)"


def _grads(n, steps, seed):
    """Gradients spread over six decades, the first step's 10x larger (so the
    running maximum of amsgrad departs from exp_avg_sq afterwards)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for k in range(steps):
        mag = 10.0 ** (torch.rand(n, generator=g) * 6.0 - 4.0)
        x = torch.randn(n, generator=g) * mag * (10.0 if k == 0 else 1.0)
        out.append(x.float())
    return out


def _params(n, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, generator=g) * 10.0 ** (torch.rand(n, generator=g) * 3.0 - 2.0)).float()


# --------------------------------------------------------------------- CPU
@pytest.mark.parametrize("hyper", HYPER)
@pytest.mark.parametrize("opts", OPTIONS)
def test_reference_is_torch_adam_in_fp64(opts, hyper):
    """The oracle of this file with un-rounded scalars is torch.optim.Adam in
    fp64 (grad_scale applied to the gradient torch is given)."""
    wd, decoupled, maximize, amsgrad, gs = opts
    lr, b1, b2, eps = hyper
    n = 257
    p0 = _params(n, 1).double()
    grads = [x.double() for x in _grads(n, 5, 2)]
    q = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([q], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, amsgrad=amsgrad,
                           maximize=maximize, decoupled_weight_decay=decoupled)
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    vmax = torch.zeros_like(p0) if amsgrad else None
    for k, g in enumerate(grads):
        q.grad = g * gs
        opt.step()
        adam_ref(p, g, m, v, vmax, k + 1, lr, b1, b2, eps, wd, decoupled, maximize, gs, round_scalars=False)
    st = opt.state[q]
    torch.testing.assert_close(p, q.detach(), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(m, st["exp_avg"], rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(v, st["exp_avg_sq"], rtol=1e-12, atol=1e-12)
    if amsgrad:
        torch.testing.assert_close(vmax, st["max_exp_avg_sq"], rtol=1e-12, atol=1e-12)


# ---------------------------------------------------------------- adam_flat
class _Flat:
    """The four (five with amsgrad) operands of adam_flat as views into padded
    device buffers filled with a sentinel, plus the fp64 reference state.
    ``offs``: element offset of each view (param, grad, exp_avg, exp_avg_sq,
    max_exp_avg_sq) in its buffer -- a multiple of 4 keeps the 16-byte
    alignment of the allocation, anything else loses it."""
    PAD = 8
    SENTINEL = -12345.678

    def __init__(self, n, amsgrad, offs=(4, 4, 4, 4, 4), seed=0, warm=False):
        self.n = n
        self.bufs = [torch.full((n + 2 * self.PAD,), self.SENTINEL, device="cuda") for _ in range(5)]
        self.views = [b[o:o + n] for b, o in zip(self.bufs, offs)]
        self.offs = offs
        p0 = _params(n, seed)
        self.views[0].copy_(p0)
        g = torch.Generator().manual_seed(seed + 100)
        m0 = (torch.randn(n, generator=g) * 0.1).float() if warm else torch.zeros(n)
        v0 = (torch.rand(n, generator=g) * 0.1).float() if warm else torch.zeros(n)
        self.views[2].copy_(m0)
        self.views[3].copy_(v0)
        self.views[4].copy_(v0)
        self.amsgrad = amsgrad
        self.ref = [p0.double(), m0.double(), v0.double(), v0.double() if amsgrad else None]
        for o, v in zip(offs, self.views):
            assert v.is_contiguous() and (v.data_ptr() % 16 == 0) == (o % 4 == 0)

    def step(self, g, step, lr, b1, b2, eps, wd, decoupled, maximize, gs, *, host_lr=None, host_step=None,
             lr_t=None, step_t=None, ticket=None, skip=None, reference=True):
        p, gv, m, v, vmax = self.views
        gv.copy_(g)
        _mod().adam_flat(p, gv, m, v, vmax if self.amsgrad else None, lr if host_lr is None else host_lr,
                         b1, b2, eps, wd, float(step if host_step is None else host_step), gs, decoupled,
                         maximize, lr_t, step_t, ticket, skip)
        torch.cuda.synchronize()
        if reference:
            rp, rm, rv, rvmax = self.ref
            adam_ref(rp, g.double(), rm, rv, rvmax, step, lr, b1, b2, eps, wd, decoupled, maximize, gs)

    def snapshot(self):
        return [b.clone() for b in self.bufs]

    def check(self, what=""):
        p, _, m, v, vmax = self.views
        rp, rm, rv, rvmax = self.ref
        _check_p(p, rp, what)
        _check_moment("m", m, rm, what)
        _check_moment("v", v, rv, what)
        if self.amsgrad:
            _check_moment("vmax", vmax, rvmax, what)
        self.check_sentinels(what)

    def check_sentinels(self, what=""):
        """Everything outside the views is bitwise what it was."""
        for k, (b, o) in enumerate(zip(self.bufs, self.offs)):
            if k == 4 and not self.amsgrad:
                continue
            outside = torch.cat([b[:o], b[o + self.n:]])
            want = torch.full_like(outside, self.SENTINEL)
            assert torch.equal(outside.view(torch.int32), want.view(torch.int32)), f"buffer {k} overrun{what}"


@gpu
@pytest.mark.parametrize("hyper", HYPER)
@pytest.mark.parametrize("opts", OPTIONS)
def test_adam_flat_option_matrix(opts, hyper):
    wd, decoupled, maximize, amsgrad, gs = opts
    n = 4099
    f = _Flat(n, amsgrad)
    for k, g in enumerate(_grads(n, 5, 7)):
        f.step(g, k + 1, *hyper, wd, decoupled, maximize, gs)
    f.check()
    if amsgrad:
        # max_exp_avg_sq == exp_avg_sq would prove nothing: exp_avg_sq is below
        # its running maximum where the later gradients are small against
        # the first one -- with magnitudes drawn afresh over six decades each
        # step that is about half the elements at either beta2
        assert (f.views[4] > f.views[3]).float().mean().item() > 0.25
    else:  # the fifth buffer was never handed to the kernel
        assert torch.equal(f.views[4], torch.zeros(n, device="cuda"))


ALIGNED = (4, 4, 4, 4, 4)
UNALIGNED = (1, 1, 1, 1, 1)
GRAD_UNALIGNED = (4, 1, 4, 4, 4)


@gpu
@pytest.mark.parametrize("amsgrad", [False, True])
@pytest.mark.parametrize("offs", [ALIGNED, UNALIGNED, GRAD_UNALIGNED], ids=["aligned", "unaligned", "grad_unaligned"])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1025])
def test_adam_flat_sizes_and_alignment(n, offs, amsgrad):
    """No vector body (n < 4), body + tail, both sides of a 256-lane workgroup
    of float4 (n = 1023 / 1025), from 16-byte aligned views and from views at a
    4-byte offset (the scalar fallback), weight decay on."""
    f = _Flat(n, amsgrad, offs)
    for k, g in enumerate(_grads(n, 2, n)):
        f.step(g, k + 1, *HYPER[1], 0.05, bool(k), False, 1.0)
        f.check(f" (n={n}, step {k + 1})")


@gpu
def test_adam_flat_grid_stride():
    """n / 4 past 4096 workgroups x 256 lanes: the float4 loop takes a second
    trip, then the three-element tail."""
    n = 4096 * 1024 + 3 * 1024 + 3
    f = _Flat(n, False)
    for k, g in enumerate(_grads(n, 2, 11)):
        f.step(g, k + 1, *HYPER[0], 1e-2, bool(k), False, 1.0)
    f.check()


@gpu
def test_adam_flat_device_lr():
    """lr_t: the device learning rate overrides the (here wrong) host one."""
    n = 4099
    f = _Flat(n, False)
    lr, b1, b2, eps = HYPER[1]
    lr_t = torch.tensor([lr], dtype=torch.float32, device="cuda")
    for k, g in enumerate(_grads(n, 3, 13)):
        f.step(g, k + 1, lr, b1, b2, eps, 1e-2, True, False, 1.0, host_lr=123.0, lr_t=lr_t)
    f.check()


@gpu
def test_adam_flat_device_step_without_ticket():
    """step_t alone: the bias corrections come from the device count (the host
    step passed is wrong on purpose) and the count is left as it was."""
    n = 4099
    f = _Flat(n, False, warm=True)
    step_t = torch.tensor([3.0], dtype=torch.float32, device="cuda")
    f.step(_grads(n, 1, 17)[0], 3, *HYPER[0], 1e-2, False, False, 1.0, host_step=1, step_t=step_t)
    f.check()
    assert float(step_t) == 3.0


@gpu
@pytest.mark.parametrize("decoupled", [False, True])
def test_adam_flat_advance_mode_matches_fp64(decoupled):
    """step_t + ticket: the launch uses device count + 1 and its last
    workgroup (of 5 here) publishes it and re-arms the ticket."""
    n = 4099
    f = _Flat(n, False, warm=True)
    step_t = torch.tensor([2.0], dtype=torch.float32, device="cuda")
    ticket = torch.zeros(1, dtype=torch.int32, device="cuda")
    for k, g in enumerate(_grads(n, 3, 19)):
        f.step(g, 3 + k, *HYPER[1], 0.05, decoupled, False, 1.0, host_step=0, step_t=step_t, ticket=ticket)
        assert float(step_t) == 3.0 + k and int(ticket) == 0
    f.check()


@gpu
def test_adam_flat_skip_word_in_advance_mode():
    """A nonzero skip word: nothing changes -- parameters, moments, the device
    step count and the ticket."""
    n = 4099
    f = _Flat(n, False, warm=True)
    step_t = torch.tensor([2.0], dtype=torch.float32, device="cuda")
    ticket = torch.zeros(1, dtype=torch.int32, device="cuda")
    skip = torch.ones(1, dtype=torch.int32, device="cuda")
    g = _grads(n, 1, 23)[0]
    f.views[1].copy_(g)
    before = f.snapshot()
    f.step(g, 3, *HYPER[1], 0.05, True, False, 1.0, host_step=0, step_t=step_t, ticket=ticket, skip=skip,
           reference=False)
    for a, b in zip(before, f.bufs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert float(step_t) == 2.0 and int(ticket) == 0
    skip.zero_()  # and the same launch with the word cleared is an ordinary step
    f.step(g, 3, *HYPER[1], 0.05, True, False, 1.0, host_step=0, step_t=step_t, ticket=ticket, skip=skip)
    f.check()
    assert float(step_t) == 3.0 and int(ticket) == 0


# ------------------------------------------------- Adam folded into the step
FOLD = dict(lr=2.5e-3, betas=(0.8, 0.95), eps=1e-6, weight_decay=0.05)


def _motion(cell, n_train, seed):
    from pytorch_distributed_rnn_amd.data.motion import synthetic_motion
    from pytorch_distributed_rnn_amd.models.motion import MotionModel
    from pytorch_distributed_rnn_amd.utils.flat import flatten_module
    torch.manual_seed(seed)
    train, _, _ = synthetic_motion(n_train=n_train, n_validation=1, n_test=1, seed=seed)
    m = MotionModel(9, 32, 2, 6, cell=cell).cuda()
    flatten_module(m)
    return m, train.features.cuda(), train.labels.cuda().reshape(-1)


@gpu
@pytest.mark.parametrize("batch", [64, 200])
@pytest.mark.parametrize("decoupled", [False, True])
@pytest.mark.parametrize("cell", ["lstm", "gru"])
def test_folded_adam_matches_fp64(cell, decoupled, batch):
    """slab_reduce_adam_kernel's Adam (one-launch step at B = 64, separate
    launches at B = 200): the update it applied equals the fp64 step from the
    state before it with the gradient that launch wrote to flat.grad."""
    from pytorch_distributed_rnn_amd.ops.adam import FusedAdam
    from pytorch_distributed_rnn_amd.train.fused_step import MotionTrainStep
    m, feats, labels = _motion(cell, 3 * batch, 31)
    opt = FusedAdam(m.parameters(), decoupled_weight_decay=decoupled, **FOLD)
    step = MotionTrainStep(m, opt, None)
    opt.materialize_state()
    fs = opt._flat_state[0]
    flat = step.flat
    assert fs["flat_p"].data_ptr() == flat.data.data_ptr()
    lr, (b1, b2), eps, wd = FOLD["lr"], FOLD["betas"], FOLD["eps"], FOLD["weight_decay"]
    for k in range(3):
        p, mm, v = flat.data.double().cpu(), fs["exp_avg"].double().cpu(), fs["exp_avg_sq"].double().cpu()
        idx = torch.arange(k * batch, (k + 1) * batch, device="cuda")
        step(feats, labels, idx)
        torch.cuda.synchronize()
        g = flat.grad.double().cpu()
        assert torch.isfinite(g).all() and g.abs().max().item() > 0
        assert float(fs["step"]) == k + 1
        adam_ref(p, g, mm, v, None, k + 1, lr, b1, b2, eps, wd, decoupled)
        what = f" ({cell}, step {k + 1})"
        _check_p(flat.data, p, what)
        _check_moment("m", fs["exp_avg"], mm, what)
        _check_moment("v", fs["exp_avg_sq"], v, what)
    assert opt.state_dict()["state"][0]["step"] == 3


@gpu
@pytest.mark.parametrize("decoupled", [False, True])
def test_folded_adam_graph_replay_matches_eager(decoupled):
    """The graph-replayed epoch (device step count, ticket) with weight decay
    on equals the eager launches: parameters, moments, step count."""
    from pytorch_distributed_rnn_amd.ops.adam import FusedAdam
    from pytorch_distributed_rnn_amd.train.fused_step import MotionTrainStep
    from pytorch_distributed_rnn_amd.utils.flat import flatten_module
    n_train, bs = 192, 64
    m1, feats, labels = _motion("lstm", n_train, 6)
    m2 = copy.deepcopy(m1)
    flatten_module(m2)
    o1 = FusedAdam(m1.parameters(), decoupled_weight_decay=decoupled, **FOLD)
    o2 = FusedAdam(m2.parameters(), decoupled_weight_decay=decoupled, **FOLD)
    s1 = MotionTrainStep(m1, o1, None, cuda_graph=True)
    s2 = MotionTrainStep(m2, o2, None)
    assert s1.cuda_graph and not s2.cuda_graph
    gen = torch.Generator().manual_seed(3)
    replays = 0
    for e in range(5):
        idx_list = list(torch.split(torch.randperm(n_train, generator=gen).cuda(), bs))
        res = s1.run_steps(feats, labels, idx_list)
        if res is None:
            res = [s1(feats, labels, i) for i in idx_list]
        else:
            replays += 1
        a = [r.clone() for r in res]
        b = [s2(feats, labels, i).clone() for i in idx_list]
        for k, (x, y) in enumerate(zip(a, b)):
            torch.testing.assert_close(x, y, rtol=1e-5, atol=1e-6, msg=lambda t: f"epoch {e} step {k}: {t}")
    assert replays >= 1, "the epoch was never replayed from a graph"
    torch.cuda.synchronize()
    assert _ratio("adam.p", s1.flat.data, s2.flat.data, 1e-5, 1e-6) <= 1.0
    f1, f2 = o1._flat_state[0], o2._flat_state[0]
    _check_moment("m", f1["exp_avg"], f2["exp_avg"])
    _check_moment("v", f1["exp_avg_sq"], f2["exp_avg_sq"])
    steps = 5 * len(idx_list)
    assert o1.state_dict()["state"][0]["step"] == o2.state_dict()["state"][0]["step"] == steps


# ------------------------------------------------------ FusedAdam as a whole
def _flat_group(shapes, seed):
    from pytorch_distributed_rnn_amd.utils.flat import FlatParameters
    g = torch.Generator().manual_seed(seed)
    ps = [torch.nn.Parameter(torch.randn(*s, generator=g).cuda()) for s in shapes]
    return ps, FlatParameters(ps)


def _double_copy(params):
    return [torch.nn.Parameter(p.detach().double().cpu().clone()) for p in params]


def _set_grads(params, refs, gen, scale=1.0):
    """The same random gradient into a GPU parameter's (flat) .grad and its
    fp64 CPU twin's."""
    for p, q in zip(params, refs):
        g = (torch.randn(p.shape, generator=gen) * scale).float()
        if p.grad is None:
            p.grad = g.cuda()
        else:
            p.grad.copy_(g)
        if q is not None:
            q.grad = g.double()


@gpu
def test_fused_adam_two_groups_match_torch_fp64():
    from pytorch_distributed_rnn_amd.ops.adam import FusedAdam
    pa, fa = _flat_group([(7, 5), (13,)], 41)
    pb, fb = _flat_group([(33,), (4, 9)], 42)
    qa, qb = _double_copy(pa), _double_copy(pb)
    ga = dict(lr=1e-2, weight_decay=1e-2)
    gb = dict(lr=3e-3, weight_decay=0.1, amsgrad=True)
    opt = FusedAdam([dict(params=pa, **ga), dict(params=pb, **gb)], betas=(0.8, 0.95), eps=1e-6)
    ref = torch.optim.Adam([dict(params=qa, **ga), dict(params=qb, **gb)], betas=(0.8, 0.95), eps=1e-6)
    gen = torch.Generator().manual_seed(43)
    for k in range(5):
        _set_grads(pa + pb, qa + qb, gen, 10.0 if k == 0 else 1.0)
        assert fa.grads_attached() and fb.grads_attached()
        opt.step()
        ref.step()
        assert opt.native_steps == 2 * (k + 1)
    torch.cuda.synchronize()
    for p, q in zip(pa + pb, qa + qb):
        _check_p(p, q)
        for key in ("exp_avg", "exp_avg_sq") + (("max_exp_avg_sq",) if any(p is x for x in pb) else ()):
            _check_moment(key, opt.state[p][key], ref.state[q][key])
        assert float(opt.state[p]["step"]) == 5
    assert (opt.state[pb[0]]["max_exp_avg_sq"] > opt.state[pb[0]]["exp_avg_sq"]).any()
    assert "max_exp_avg_sq" not in opt.state[pa[0]]


@gpu
def test_fused_adam_resume_is_bitwise():
    """3 steps, state_dict() into a fresh FusedAdam on a copy of the model, 2
    more steps == 5 uninterrupted steps, bit for bit (amsgrad on)."""
    from pytorch_distributed_rnn_amd.ops.adam import FusedAdam
    from pytorch_distributed_rnn_amd.utils.flat import FlatParameters
    torch.manual_seed(51)
    kw = dict(lr=1e-2, betas=(0.8, 0.95), eps=1e-6, weight_decay=1e-2, amsgrad=True)
    ma = torch.nn.Sequential(torch.nn.Linear(9, 32), torch.nn.Linear(32, 6)).cuda()
    mb = copy.deepcopy(ma)
    gen = torch.Generator().manual_seed(52)
    grads = [[(torch.randn(p.shape, generator=gen) * (10.0 if k == 0 else 1.0)).cuda() for p in ma.parameters()]
             for k in range(5)]

    def run(model, opt, steps):
        flat = FlatParameters(list(model.parameters()))
        for k in steps:
            for p, g in zip(model.parameters(), grads[k]):
                p.grad.copy_(g)
            assert flat.grads_attached()
            opt.step()
        return opt

    oa = run(ma, FusedAdam(ma.parameters(), **kw), range(5))
    ob = run(mb, FusedAdam(mb.parameters(), **kw), range(3))
    sd = copy.deepcopy(ob.state_dict())
    mc = copy.deepcopy(mb)
    for p in mc.parameters():
        p.grad = None
    oc = FusedAdam(mc.parameters(), **kw)
    oc.load_state_dict(sd)
    run(mc, oc, range(3, 5))
    torch.cuda.synchronize()
    assert oa.native_steps == 5 and oc.native_steps == 2
    sa, sc = oa.state_dict()["state"], oc.state_dict()["state"]
    for i, (p, q) in enumerate(zip(ma.parameters(), mc.parameters())):
        assert torch.equal(p.detach().view(torch.int32), q.detach().view(torch.int32))
        assert float(sa[i]["step"]) == float(sc[i]["step"]) == 5
        for key in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"):
            assert torch.equal(sa[i][key].view(torch.int32), sc[i][key].view(torch.int32)), (i, key)
    assert (sa[0]["max_exp_avg_sq"] > sa[0]["exp_avg_sq"]).any()


@gpu
def test_fused_adam_scattered_group_takes_reference_path():
    """Parameters that are not one contiguous span: torch's own step for that
    group -- still the fp64 result, and a nonzero skip word leaves it alone."""
    from pytorch_distributed_rnn_amd.ops.adam import FusedAdam
    from pytorch_distributed_rnn_amd.utils.flat import contiguous_span
    g = torch.Generator().manual_seed(61)
    ps = [torch.nn.Parameter(torch.randn(10, 3, generator=g).cuda()), torch.nn.Parameter(torch.randn(7, generator=g).cuda())]
    assert contiguous_span([p.data for p in ps]) is None
    qs = _double_copy(ps)
    kw = dict(lr=1e-2, betas=(0.8, 0.95), eps=1e-6, weight_decay=1e-2)
    opt, ref = FusedAdam(ps, **kw), torch.optim.Adam(qs, **kw)
    gen = torch.Generator().manual_seed(62)
    _set_grads(ps, [None, None], gen)
    before = [p.detach().clone() for p in ps]
    opt.step(skip=torch.ones(1, dtype=torch.int32, device="cuda"))
    for p, b in zip(ps, before):
        assert torch.equal(p.detach().view(torch.int32), b.view(torch.int32))
    assert not opt.state[ps[0]]
    for _ in range(5):
        _set_grads(ps, qs, gen)
        opt.step(skip=torch.zeros(1, dtype=torch.int32, device="cuda"))
        ref.step()
    assert getattr(opt, "native_steps", 0) == 0
    for p, q in zip(ps, qs):
        _check_p(p, q)
        _check_moment("m", opt.state[p]["exp_avg"], ref.state[q]["exp_avg"])
        _check_moment("v", opt.state[p]["exp_avg_sq"], ref.state[q]["exp_avg_sq"])


# ---------------------------------------------------------------- clip_flat
def _clip_ref(g, max_norm, eps):
    norm = g.double().norm().item()
    return min(1.0, max_norm / (norm + eps)), norm


@gpu
def test_clip_flat_below_max_norm_is_identity():
    g = _grads(1000, 1, 71)[0].cuda() * 1e-5
    g0 = g.clone()
    scale, norm = _clip_ref(g, 1.0, 1e-6)
    assert norm < 0.5 and scale == 1.0
    out = _mod().clip_flat(g, 1.0, 1e-6)
    torch.cuda.synchronize()
    assert out[0].item() == 1.0
    assert torch.equal(g.view(torch.int32), g0.view(torch.int32))
    torch.testing.assert_close(out[1].item(), norm, rtol=1e-5, atol=0)


@gpu
def test_clip_flat_zero_gradient():
    g = torch.zeros(5000, device="cuda")
    out = _mod().clip_flat(g, 1.0, 1e-6)
    torch.cuda.synchronize()
    assert out[0].item() == 1.0 and out[1].item() == 0.0
    assert torch.equal(g, torch.zeros_like(g))


@gpu
@pytest.mark.parametrize("n", [1, 1024 * 4096 + 777])
def test_clip_flat_sizes(n):
    """One element, and past 1024 partials x 4096 elements (the partial count
    is capped, so the sum-of-squares pass strides)."""
    g = (torch.randn(n, generator=torch.Generator().manual_seed(n)) * 3.0).float().cuda()
    g[0] = -3.0
    g0 = g.double().cpu()
    scale, norm = _clip_ref(g0, 1.0, 1e-6)
    assert scale < 1.0
    out = _mod().clip_flat(g, 1.0, 1e-6)
    torch.cuda.synchronize()
    torch.testing.assert_close(out[0].item(), scale, rtol=1e-5, atol=0)
    torch.testing.assert_close(out[1].item(), norm, rtol=1e-5, atol=0)
    torch.testing.assert_close(g.double().cpu(), g0 * scale, rtol=1e-5, atol=0)
