"""The objectives of the fused training step on the GPU (csrc/objective.hip, dbsr_amd.objectives,
DBSRTrainer(objective=...)) against values computed on the host: the reference's own float64 results
(tests/golden/objective.npz) for the kernels, autograd through the oracle for the trainer.  No torch convolution
runs on the device here.

Bounds, none of them taken from the code under test: a float32 result may be off its float64 value by
max(2 x the reference's own float32-vs-float64 error stored in the fixture, 4 float32 ulp of the quantity's
magnitude) -- the same arithmetic, possibly summed in another order.  Every test prints what it measured.

This file is not collected into the suite: tests/test_gpu_objective.py runs it in a process of its own and reports
every case (it says why).  To run it directly: python -m pytest -m gpu tests/gpu_objective_cases.py"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = 'cuda'
BI = 40
METRICS = ('l1', 'l2', 'l2_sqrt', 'charbonnier')
CASES = [('a', 3), ('b', 0), ('c', 4)]
NOISE = 'merging.weight_predictor.4.0.bias'      # exact gradient 0 (softmax shift invariance): rounding noise


def _bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def ulp32(x):
    return float(np.spacing(np.float32(abs(float(x)))))


def bound(err_ref, magnitude):
    return max(2.0 * float(err_ref), 4.0 * ulp32(magnitude))


def inputs(g, tag):
    if tag == 'b':
        return torch.from_numpy(g['b_pred_q']).float() / 256.0, torch.from_numpy(g['b_gt_q']).float() / 256.0
    return torch.from_numpy(g[tag + '_pred']), torch.from_numpy(g[tag + '_gt'])


def full_grad(g, key, shape, bi):
    """The fixture's crop-only float64 gradient placed in a zero [B,3,H,W] tensor."""
    out = torch.zeros(shape, dtype=torch.float64)
    (out[..., bi:-bi, bi:-bi] if bi else out).copy_(torch.from_numpy(g[key + '_grad64']))
    return out


@pytest.fixture(scope='module')
def ops():
    from dbsr_amd import ops as O
    return O


# ----------------------------------------------------------------------------------------------------
# kernels
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('metric', METRICS)
@pytest.mark.parametrize('tag,bi', CASES)
def test_step_vs_fixture(golden, ops, tag, bi, metric):
    """dbsr_objective_step, fp32 dpre: the loss, the gated gradient (weight 1, then weight 0.5 with an upstream
    gradient) and the per-image statistics."""
    g = golden('objective')
    pred, gt = inputs(g, tag)
    key = '%s_%s' % (tag, metric)
    ref = full_grad(g, key, pred.shape, bi)
    gate = (pred > 0).double()
    loss, dpre, stats = ops.objective_step(pred.to(DEV), gt.to(DEV), bi, metric)
    got = dpre[..., :3].permute(0, 3, 1, 2).double().cpu()
    e_l = abs(float(loss[0]) - float(g[key + '_loss64']))
    e_g = float((got - gate * ref).abs().max())
    b_l, b_g = bound(g[key + '_err_loss'], g[key + '_loss64']), bound(g[key + '_err_grad'], ref.abs().max())
    print('%s: loss err %.3e (bound %.3e)  grad err %.3e (bound %.3e)' % (key, e_l, b_l, e_g, b_g))
    assert e_l <= b_l and e_g <= b_g
    assert float(loss[1]) == float(loss[0]) and float(dpre[..., 3:].abs().max()) == 0.0
    d = (pred.double() - gt.double())
    d = d[..., bi:-bi, bi:-bi] if bi else d
    sq = (d * d).sum(dim=(1, 2, 3))
    st = stats.cpu()
    assert float(((st[:, 0] - sq).abs() / sq).max()) <= 1e-6
    assert st[:, 1].tolist() == [float(d[0].numel())] * pred.shape[0]
    # weight and an upstream gradient, added before the gate
    gen = torch.Generator().manual_seed(5)
    ge = torch.randn(pred.shape, generator=gen) * float(ref.abs().max())
    loss2, dpre2, _ = ops.objective_step(pred.to(DEV), gt.to(DEV), bi, metric, weight=0.5, gextra=ge.to(DEV))
    inside = torch.zeros(pred.shape, dtype=torch.float64)
    (inside[..., bi:-bi, bi:-bi] if bi else inside).fill_(1.0)
    want = gate * inside * (0.5 * ref + ge.double())
    e2 = float((dpre2[..., :3].permute(0, 3, 1, 2).double().cpu() - want).abs().max())
    b2 = bound(g[key + '_err_grad'], want.abs().max())
    print('   weight 0.5 + gextra: grad err %.3e (bound %.3e)' % (e2, b2))
    assert e2 <= b2
    assert abs(float(loss2[1]) - 0.5 * float(g[key + '_loss64'])) <= b_l and float(loss2[0]) == float(loss[0])


@pytest.mark.parametrize('dt,ld,scale', [(torch.bfloat16, 8, None), (torch.bfloat16, 16, None),
                                          (torch.float16, 8, 1024.0), (torch.float16, 16, 1024.0)])
def test_step_16bit_dpre_within_one_ulp(golden, ops, dt, ld, scale):
    """Both 16-bit layouts (ld 8: one 16-B store per pixel; generic) round the fp32 path's value once."""
    g = golden('objective')
    pred, gt = inputs(g, 'b')
    p, q = pred.to(DEV), gt.to(DEV)
    gen = torch.Generator().manual_seed(6)
    ge = (torch.randn(pred.shape, generator=gen) * 1e-5).to(DEV)
    bits = 7 if dt == torch.bfloat16 else 10                      # stored mantissa bits
    tiny = 2.0 ** -133 if dt == torch.bfloat16 else 2.0 ** -24    # the smallest subnormal
    for metric in METRICS:
        st = ops.loss_scale_state(scale, DEV) if scale else None
        _, d32, _ = ops.objective_step(p, q, 0, metric, gextra=ge, state=st)
        _, d16, _ = ops.objective_step(p, q, 0, metric, gextra=ge, state=st, dpre_dtype=dt, ld=ld)
        x = d32[..., :3]
        err = (d16[..., :3].float() - x).abs()
        ulp = torch.ldexp(torch.ones_like(x), torch.frexp(x)[1] - 1 - bits).clamp(min=tiny)    # of the 16-bit format
        assert bool((err <= ulp).all()), (metric, float((err / ulp).max()))
        assert float(d16[..., 3:].float().abs().max()) == 0.0 and float(d32.abs().max()) > 0
    # a product beyond fp16's range is stored as inf, never saturated
    if dt == torch.float16:
        _, dh, _ = ops.objective_step(p, q, 0, 'l2', state=ops.loss_scale_state(2.0 ** 40, DEV), dpre_dtype=dt, ld=ld)
        assert bool(torch.isinf(dh).any()) and not bool(torch.isnan(dh).any())


@pytest.mark.parametrize('tag,bi', [('a', 3), ('b', 0), ('b', 7)])
def test_l1_bitwise_equals_l1_loss_backward(golden, ops, tag, bi):
    """Metric l1, weight 1, no gextra: the loss and dpre of dbsr_l1_loss_backward, and of _scaled at 1 and 1024."""
    g = golden('objective')
    pred, gt = inputs(g, tag)
    p, q = pred.to(DEV), gt.to(DEV)
    for dt, ld in ((torch.float32, 8), (torch.float16, 8), (torch.float16, 16), (torch.bfloat16, 8)):
        for scale in (None, 1.0, 1024.0):
            st = ops.loss_scale_state(scale, DEV) if scale else None
            l0, d0 = ops.l1_loss_backward(p, q, bi, dt, ld, state=st)
            l1, d1, _ = ops.objective_step(p, q, bi, 'l1', state=st, dpre_dtype=dt, ld=ld)
            assert torch.equal(_bits(l0), _bits(l1[:1])), (dt, ld, scale)
            assert torch.equal(_bits(d0), _bits(d1)), (dt, ld, scale)
            assert float(d0.float().abs().max()) > 0


def test_two_runs_bitwise_equal(golden, ops):
    g = golden('objective')
    pred, gt = inputs(g, 'b')
    p, q = pred.to(DEV), gt.to(DEV)
    ge = (torch.randn(pred.shape, generator=torch.Generator().manual_seed(7)) * 1e-5).to(DEV)
    for metric in METRICS:
        for dt in (torch.float32, torch.bfloat16):
            r = [ops.objective_step(p, q, 2, metric, weight=0.7, gextra=ge, dpre_dtype=dt) for _ in range(2)]
            assert torch.equal(r[0][0], r[1][0]) and torch.equal(_bits(r[0][1]), _bits(r[1][1]))
            assert torch.equal(r[0][2], r[1][2])
        f = [ops.objective_forward(p, q, 2, metric) for _ in range(2)]
        assert all(torch.equal(a, b) for a, b in zip(f[0], f[1]))


def test_l2_sqrt_zero_distance_pixel_is_zero(ops):
    """Where all three differences are zero torch autograd gives NaN; the kernels give 0."""
    gen = torch.Generator().manual_seed(8)
    gt = 0.1 + 0.8 * torch.rand(1, 3, 12, 11, generator=gen)
    pred = gt + 0.05
    pred[0, :, 5, 6] = gt[0, :, 5, 6]
    p = pred.clone().requires_grad_(True)
    (((p - gt) ** 2).sum(dim=-3)).sqrt().mean().backward()
    assert bool(torch.isnan(p.grad[0, :, 5, 6]).all())                          # the deviation is real
    _, dpre, _ = ops.objective_step(pred.to(DEV), gt.to(DEV), 1, 'l2_sqrt')
    _, gun, _ = ops.objective_forward(pred.to(DEV), gt.to(DEV), 1, 'l2_sqrt')
    for t in (dpre[0, 5, 6, :3], gun[0, :, 5, 6]):
        assert float(t.abs().max()) == 0.0
    assert bool(torch.isfinite(dpre).all()) and bool(torch.isfinite(gun).all())
    assert float(dpre[0, 5, 5, :3].abs().min()) > 0


def test_psnr_vs_fixture_and_drop_rule(golden):
    from dbsr_amd import objectives as obj
    g = golden('objective')
    for tag, bi in CASES:
        pred, gt = inputs(g, tag)
        v = float(obj.PSNR(bi or None)(pred.to(DEV), gt.to(DEV)))
        vm = float(obj.PSNR(bi or None, max_value=None)(pred.to(DEV), gt.to(DEV)))
        b = bound(g[tag + '_psnr_err'], g[tag + '_psnr64'])
        print('%s: psnr err %.3e, gt-max err %.3e (bound %.3e)' % (tag, abs(v - float(g[tag + '_psnr64'])),
                                                                   abs(vm - float(g[tag + '_psnr_gtmax64'])), b))
        assert abs(v - float(g[tag + '_psnr64'])) <= b and abs(vm - float(g[tag + '_psnr_gtmax64'])) <= b
    pred, gt = inputs(g, 'a')
    valid = torch.from_numpy(g['a_valid'])
    b = bound(g['a_psnr_err'], g['a_psnr64'])
    assert abs(float(obj.PSNR(3)(pred.to(DEV), gt.to(DEV), valid.to(DEV))) - float(g['a_psnrm64'])) <= b
    drop = pred.clone()
    drop[1] = gt[1]                                               # image 1 is dropped: the mean of the rest
    assert abs(float(obj.PSNR(3)(drop.to(DEV), gt.to(DEV))) - float(g['a_psnr_drop64'])) <= b
    _, cg = inputs(g, 'c')
    assert float(obj.PSNR(4)(cg.to(DEV), cg.to(DEV))) == 0.0      # every image dropped


@pytest.mark.parametrize('tag,bi', CASES)
def test_module_autograd_vs_fixture(golden, tag, bi):
    """objectives.PixelWiseError on device tensors: the loss and, through autograd, dloss/dpred (ungated)."""
    from dbsr_amd import objectives as obj
    g = golden('objective')
    pred, gt = inputs(g, tag)
    keys = [(m, '%s_%s' % (tag, m), None) for m in METRICS]
    if tag == 'a':
        valid = torch.from_numpy(g['a_valid']).to(DEV)
        keys += [('l1', 'a_l1m', valid), ('l2', 'a_l2m', valid)]
    for metric, key, valid in keys:
        p = pred.to(DEV).requires_grad_(True)
        loss = obj.PixelWiseError(metric, bi or None)(p, gt.to(DEV), valid=valid)
        (3.0 * loss).backward()
        ref = full_grad(g, key, pred.shape, bi)
        e_l = abs(float(loss) - float(g[key + '_loss64']))
        e_g = float((p.grad.double().cpu() / 3.0 - ref).abs().max())
        b_l, b_g = bound(g[key + '_err_loss'], g[key + '_loss64']), bound(g[key + '_err_grad'], ref.abs().max())
        print('%s: loss err %.3e (bound %.3e)  grad err %.3e (bound %.3e)' % (key, e_l, b_l, e_g, b_g))
        assert e_l <= b_l and e_g <= b_g
    if tag == 'a':
        v = obj.masked_mse(pred.to(DEV), gt.to(DEV), valid, 3)
        assert abs(float(v) - float(g['a_al2_loss64'])) <= bound(g['a_l2m_err_loss'], g['a_al2_loss64'])
        with pytest.raises(ValueError, match='valid mask'):
            obj.PixelWiseError('charbonnier', 3)(pred.to(DEV), gt.to(DEV), valid=valid)


def test_relu_grad_scaled(ops):
    gen = torch.Generator().manual_seed(9)
    pred = torch.rand(2, 3, 19, 23, generator=gen) - 0.3
    gout = torch.randn(2, 3, 19, 23, generator=gen)
    st = ops.loss_scale_state(1024.0, DEV)
    dpre = ops.relu_grad_scaled(pred.to(DEV), gout.to(DEV), st, torch.zeros(2, 19, 23, 8, device=DEV))
    want = torch.where(pred > 0, gout * 1024.0, torch.zeros(())).permute(0, 2, 3, 1)
    assert torch.equal(dpre[..., :3].cpu(), want) and float(dpre[..., 3:].abs().max()) == 0.0
    one = ops.loss_scale_state(1.0, DEV)
    for dt in (torch.float16, torch.bfloat16):
        a = ops.relu_grad_scaled(pred.to(DEV), gout.to(DEV), one, torch.zeros(2, 19, 23, 8, dtype=dt, device=DEV))
        b = ops.relu_grad(pred.to(DEV), gout.to(DEV), torch.zeros(2, 19, 23, 8, dtype=dt, device=DEV))
        assert torch.equal(_bits(a), _bits(b))
    big = ops.relu_grad_scaled(pred.to(DEV), gout.to(DEV), ops.loss_scale_state(2.0 ** 40, DEV),
                               torch.zeros(2, 19, 23, 8, dtype=torch.float16, device=DEV))
    assert bool(torch.isinf(big).any()) and not bool(torch.isnan(big).any())


# ----------------------------------------------------------------------------------------------------
# the trainer: the full synthetic net at 1 x 3 x 24 x 32, sr_factor 8 (tests/test_gpu_train.py's shape)
# ----------------------------------------------------------------------------------------------------
SHAPE = (1, 3, 24, 32)


def _trainer(synth_sd, dtype, **kw):
    import dbsr_amd
    from dbsr_amd.training import DBSRTrainer
    net = dbsr_amd.dbsrnet_cvpr2021(**dbsr_amd.DBSR_SYNTHETIC_KWARGS)
    net.load_state_dict(synth_sd)
    net = net.to(DEV).set_compute_dtype(dtype)
    return net, DBSRTrainer(net, boundary_ignore=BI, **kw)


_ORACLE = {}


def _crop(t):
    return t[..., BI:-BI, BI:-BI]


def _losses():
    return {'l2': lambda p, q: F.mse_loss(_crop(p), _crop(q)),
            'charbonnier': lambda p, q: ((_crop(p) - _crop(q)) ** 2 + 1e-3 ** 2).sqrt().mean()}


def _oracle(synth_sd):
    """(burst, gt, oracle pred, {metric: (loss, gradients)}): one oracle forward, one backward per metric."""
    if not _ORACLE:
        from oracle import dbsr_oracle as orc
        from dbsr_amd.burst import synthetic_bursts
        burst, gt = synthetic_bursts(*SHAPE, sr_factor=8, seed=17)
        sd = {k: v.clone().requires_grad_(not k.startswith('encoder.alignment_net')) for k, v in synth_sd.items()}
        pred, _ = orc.dbsr_forward(burst, sd)
        res = {}
        for name, fn in _losses().items():
            for v in sd.values():
                v.grad = None
            loss = fn(pred, gt)
            loss.backward(retain_graph=True)
            res[name] = (float(loss.detach()), {k: v.grad.clone() for k, v in sd.items() if v.grad is not None})
        _ORACLE.update(burst=burst, gt=gt, pred=pred.detach(), res=res)
    return _ORACLE


def _figures(tr, loss, ref_loss, ref_g):
    mine = {k: v.cpu() for k, v in tr.grads().items()}
    assert set(mine) == set(ref_g), set(mine) ^ set(ref_g)
    gmax = max(float(x.abs().max()) for x in ref_g.values())
    rel, cos = [], []
    for k, x in ref_g.items():
        if k == NOISE:
            assert float(mine[k].abs().max()) <= 1e-4 * gmax
            continue
        rel.append(float((mine[k] - x).abs().max() / x.abs().max().clamp_min(1e-12)))
        cos.append(1 - float(F.cosine_similarity(mine[k].double().flatten(), x.double().flatten(), dim=0)))
    return max(rel), max(cos), abs(loss - ref_loss)


_BUILTIN = {}


def _builtin(synth_sd, metric):
    """The built-in metric's figures against the oracle (and the trainer's statistics), computed once."""
    if metric not in _BUILTIN:
        o = _oracle(synth_sd)
        net, tr = _trainer(synth_sd, torch.float32, objective=metric)
        loss, pred = tr.forward_backward(o['burst'].to(DEV), o['gt'].to(DEV))
        torch.cuda.synchronize()
        ref_loss, ref_g = o['res'][metric]
        _BUILTIN[metric] = (_figures(tr, float(loss), ref_loss, ref_g), tr.last_stats, pred.detach().cpu(),
                            [op[2] for op in tr.plans[SHAPE].ops])
    return _BUILTIN[metric]


def test_trainer_l1_objective_is_todays_plan(synth_sd):
    """objective='l1': the same op names, and the loss and flat_grad bitwise those of objective=None."""
    o = _oracle(synth_sd)
    b, g = o['burst'].to(DEV), o['gt'].to(DEV)
    net0, tr0 = _trainer(synth_sd, torch.float32)
    net1, tr1 = _trainer(synth_sd, torch.float32, objective='l1')
    l0, _ = tr0.forward_backward(b, g)
    l1, _ = tr1.forward_backward(b, g)
    torch.cuda.synchronize()
    assert [op[2] for op in tr0.plans[SHAPE].ops] == [op[2] for op in tr1.plans[SHAPE].ops]
    assert tr0.last_stats is None
    assert torch.equal(_bits(l0), _bits(l1)) and torch.equal(_bits(tr0.flat_grad), _bits(tr1.flat_grad))
    assert float(tr0.flat_grad.abs().max()) > 0
    st = tr1.last_stats
    assert set(st) == {'Loss/total', 'Loss/rgb', 'Loss/raw/rgb', 'Stat/psnr'} and all(v.is_cuda for v in st.values())
    assert float(st['Loss/total']) == float(l1) == float(st['Loss/raw/rgb'])


@pytest.mark.parametrize('metric', ['l2', 'charbonnier'])
def test_trainer_metric_grads_vs_oracle(synth_sd, metric):
    """Whole-step gradients against autograd through the oracle with that loss, at the bounds of
    test_train_step_grads_vs_oracle (fp32); Stat/psnr against evaluation.PSNR on the step's prediction in float64."""
    from dbsr_amd import evaluation as ev
    o = _oracle(synth_sd)
    (rel, cos, lerr), stats, pred, names = _builtin(synth_sd, metric)
    ref_loss = o['res'][metric][0]
    print('%s: max-rel %.3e  1-cos %.3e  loss err %.3e (loss %.6g)' % (metric, rel, cos, lerr, ref_loss))
    assert metric + '_loss_bwd' in names and 'l1_loss_bwd' not in names
    assert lerr <= 1e-5 * max(1.0, abs(ref_loss))
    assert rel <= 2e-2 and cos <= 1e-4
    want = float(ev.PSNR(boundary_ignore=BI)(pred.double(), o['gt'].double()))
    p32 = float(ev.PSNR(boundary_ignore=BI)(pred, o['gt']))
    e = abs(float(stats['Stat/psnr']) - want)
    print('   Stat/psnr %.6f, err %.3e (bound %.3e)' % (want, e, bound(abs(p32 - want), want)))
    assert e <= bound(abs(p32 - want), want)


def test_trainer_extra_callable_matches_builtin(synth_sd):
    """An `extra` callable computing the same l2 in torch (the metric's own weight 0): its error against the oracle
    is at most 1.5 x the built-in 'l2''s."""
    from dbsr_amd.objectives import Objective
    o = _oracle(synth_sd)
    (rel0, cos0, lerr0), _, _, _ = _builtin(synth_sd, 'l2')
    calls = []

    def extra(p, q):
        calls.append(p.requires_grad and p.is_leaf)
        return F.mse_loss(_crop(p), _crop(q))

    net, tr = _trainer(synth_sd, torch.float32, objective=Objective('l2', weight=0.0, extra=extra, boundary_ignore=BI))
    loss, _ = tr.forward_backward(o['burst'].to(DEV), o['gt'].to(DEV))
    torch.cuda.synchronize()
    ref_loss, ref_g = o['res']['l2']
    rel, cos, lerr = _figures(tr, float(loss), ref_loss, ref_g)
    print('extra l2: max-rel %.3e (built-in %.3e)  1-cos %.3e (built-in %.3e)  loss err %.3e' % (rel, rel0, cos, cos0, lerr))
    assert calls == [True]                                        # pred is a leaf over the plan's buffer
    assert rel <= 1.5 * rel0 and lerr <= 1e-5 * max(1.0, abs(ref_loss))
    assert abs(float(tr.last_stats['Loss/extra']) - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss))


def test_trainer_ssim_term_graph_equals_eager(synth_sd):
    """Objective('l1', ssim=0.2): three steps, the second captured and the third replayed as HIP graphs, against a
    trainer that runs every step eagerly: losses and parameters bitwise."""
    from dbsr_amd.objectives import Objective
    o = _oracle(synth_sd)
    b, g = o['burst'].to(DEV), o['gt'].to(DEV)
    res = {}
    for graph in (True, False):
        net, tr = _trainer(synth_sd, torch.float32, objective=Objective('l1', ssim=0.2, boundary_ignore=BI))
        tr.use_graph = graph
        out = []
        for _ in range(3):
            loss = tr.step(b, g)
            out.append((loss.clone(), tr.flat.detach().clone()))
        torch.cuda.synchronize()
        plan = tr.plans[SHAPE]
        assert (plan.graphs is not None) == graph
        names = [op[2] for op in plan.ops]
        assert names[plan.obj_op - 2:plan.obj_op + 1] == ['ssim_fwd', 'ssim_bwd', 'l1_loss_bwd']
        st = tr.last_stats
        assert float(st['Loss/total']) == pytest.approx(float(st['Loss/rgb']) + float(st['Loss/ssim']), rel=1e-6)
        assert 0.0 < float(st['Loss/raw/ssim']) < 1.0
        res[graph] = out
    for (la, fa), (lb, fb) in zip(res[True], res[False]):
        assert torch.equal(_bits(la), _bits(lb)) and torch.equal(_bits(fa), _bits(fb))
    assert not torch.equal(res[True][0][1], res[True][2][1])


def _lpips_extra():
    from dbsr_amd import evaluation as ev
    sd = ev.generate_lpips_state_dict('alex', seed=0)
    lp = ev.LPIPS(boundary_ignore=BI, type='alex', weights=sd, differentiable=True).to(DEV)
    return lambda p, q: 0.1 * lp(p, q)


def test_trainer_fp16_lpips_extra_step(synth_sd):
    """fp16, dynamic scaling, extra = 0.1 LPIPS(alex, seeded weights, differentiable): finite gradients and no
    overflow at the initial scale; one step is applied."""
    from dbsr_amd.objectives import Objective
    o = _oracle(synth_sd)
    b, g = o['burst'].to(DEV), o['gt'].to(DEV)
    net, tr = _trainer(synth_sd, torch.float16, objective=Objective('l1', extra=_lpips_extra(), boundary_ignore=BI))
    loss, _ = tr.forward_backward(b, g)
    torch.cuda.synchronize()
    assert not tr.found_inf() and bool(torch.isfinite(tr.flat_grad).all()) and float(tr.flat_grad.abs().max()) > 0
    st = tr.last_stats
    assert float(st['Loss/extra']) > 0 and float(loss) == pytest.approx(float(st['Loss/rgb']) + float(st['Loss/extra']))
    before = tr.flat.detach().clone()
    tr.step(b, g)
    torch.cuda.synchronize()
    assert tr.loss_scale_state() == dict(scale=65536.0, growth_tracker=1, steps=1, skipped=0)
    assert not torch.equal(tr.flat, before) and bool(torch.isfinite(tr.flat).all())


def test_trainer_fp16_overflow_step_is_skipped(synth_sd):
    """init_scale 2^40 with an objective: the step is skipped, the weights are unchanged, the scale has backed off
    (tests/test_gpu_loss_scale.py::test_overflow_step_is_skipped with the new op)."""
    from dbsr_amd.objectives import Objective
    o = _oracle(synth_sd)
    b, g = o['burst'].to(DEV), o['gt'].to(DEV)
    net, tr = _trainer(synth_sd, torch.float16, init_scale=2.0 ** 40,
                       objective=Objective('l1', extra=_lpips_extra(), boundary_ignore=BI))
    before = [t.detach().clone() for t in (tr.flat, tr.exp_avg, tr.exp_avg_sq)]
    loss = tr.step(b, g)
    torch.cuda.synchronize()
    assert np.isfinite(float(loss))                               # the loss itself is not scaled
    for a, c in zip((tr.flat, tr.exp_avg, tr.exp_avg_sq), before):
        assert torch.equal(_bits(a), _bits(c))
    assert tr.loss_scale_state() == dict(scale=2.0 ** 39, growth_tracker=0, steps=0, skipped=1)


def test_trainer_refusals(synth_sd):
    import dbsr_amd
    from dbsr_amd.objectives import Objective
    from dbsr_amd.training import DBSRTrainer
    net = dbsr_amd.dbsrnet_cvpr2021(**dbsr_amd.DBSR_SYNTHETIC_KWARGS)
    net.load_state_dict(synth_sd)
    net = net.to(DEV)
    with pytest.raises(ValueError, match='optimizer=False'):
        DBSRTrainer(net, optimizer=False, objective='l2')
    with pytest.raises(ValueError, match='unknown metric'):
        DBSRTrainer(net, objective='huber')
    net2 = dbsr_amd.dbsrnet_cvpr2021(**dict(dbsr_amd.DBSR_SYNTHETIC_KWARGS, train_alignmentnet=True))
    net2.load_state_dict(synth_sd)
    with pytest.raises(NotImplementedError, match='extra'):
        DBSRTrainer(net2.to(DEV), alignment_grad=True, objective=Objective('l1', extra=lambda p, q: (p - q).mean()))


def _ddp_worker(rank, world, port, sd_path, data_path, out_path):
    """One rank of a 2-process run over gloo, both ranks on cuda:0, objective 'charbonnier': two steps on this
    rank's burst of the global batch (tests/test_gpu_train.py::_ddp_worker's harness)."""
    import os
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        sd = torch.load(sd_path, weights_only=True)
        data = torch.load(data_path, weights_only=True)
        net, tr = _trainer(sd, torch.float32, objective='charbonnier')
        assert tr.world == world
        b, g = data['burst'][rank:rank + 1].to(DEV), data['gt'][rank:rank + 1].to(DEV)
        losses = [float(tr.step(b, g)) for _ in range(2)]
        torch.cuda.synchronize()
        torch.save({'flat': tr.flat.cpu(), 'grad': tr.flat_grad.cpu(), 'losses': losses}, out_path % rank)
    finally:
        dist.destroy_process_group()


def test_two_ranks_charbonnier_equal_one_process(synth_sd, tmp_path):
    import socket
    import torch.multiprocessing as mp
    from dbsr_amd.burst import synthetic_bursts
    burst, gt = synthetic_bursts(2, 3, 24, 32, sr_factor=8, seed=29)
    sd_path, data_path = str(tmp_path / 'sd.pt'), str(tmp_path / 'data.pt')
    torch.save(dict(synth_sd), sd_path)
    torch.save({'burst': burst, 'gt': gt}, data_path)
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        port = sk.getsockname()[1]
    out = str(tmp_path / 'rank%d.pt')
    mp.start_processes(_ddp_worker, args=(2, port, sd_path, data_path, out), nprocs=2, join=True,
                       start_method='spawn')
    ranks = [torch.load(out % r, weights_only=True) for r in range(2)]
    torch.testing.assert_close(ranks[0]['flat'], ranks[1]['flat'], rtol=0, atol=0)      # replicas stay in sync
    net, tr = _trainer(synth_sd, torch.float32, objective='charbonnier')
    b, g = burst.to(DEV), gt.to(DEV)
    losses = [float(tr.step(b, g)) for _ in range(2)]
    torch.cuda.synchronize()
    for i in range(2):
        assert (ranks[0]['losses'][i] + ranks[1]['losses'][i]) / 2 == pytest.approx(losses[i], rel=1e-5)
    ref = tr.flat_grad.cpu()
    assert float((ranks[0]['grad'] / 2 - ref).abs().max()) <= 1e-4 * float(ref.abs().max())
    diff = (ranks[0]['flat'] - tr.flat.cpu()).abs()
    assert float(diff.max()) <= 2 * tr.lr * 1.01
    assert float((diff > 2e-2 * tr.lr).float().mean()) <= 1e-3, float((diff > 2e-2 * tr.lr).float().mean())
