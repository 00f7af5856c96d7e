"""fp16 training with device-side dynamic loss scaling (csrc/loss_scale.hip, DBSRTrainer(loss_scale=...)).

Ops: the scaled L1 backward against dbsr_l1_loss_backward (bitwise at scale 1, an exact power-of-two multiple
otherwise), the unscale + overflow check against a torch fp32 multiply by the same reciprocal (bitwise), the
guarded Adam + scaler update against torch.optim.Adam / torch.amp.GradScaler's rule.
Whole step: an fp32 trainer with a power-of-two scale against the unscaled one (scaling by 2^16 is exact in fp32 and
the backward is linear in dP: only subnormal flushes differ), the fp16 trainer's gradients against the oracle's
fp32 autograd with the existing bf16 path as the bar (fp16 carries three more mantissa bits: with working scaling it
is no worse than bf16 on the worst 1-cos, the worst max-rel and the loss error, and inside bf16's bounds of
test_gpu_train.py), the overflow skip, a dynamic run over graph replays, torch.amp.GradScaler over the autograd path,
and two ranks taking the same decisions.

Measured on an MI355X (printed by test_fp16_grads_vs_oracle; DESIGN.md 'fp16 training'): see that section."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = 'cuda'
BI = 40
NOISE = 'merging.weight_predictor.4.0.bias'      # exact gradient 0 (softmax shift invariance): rounding noise


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


def _bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


@pytest.fixture(scope='module')
def ops():
    from dbsr_amd import ops as O
    return O


def _state(st):
    from dbsr_amd import _lib as L
    w = st.cpu()
    return dict(scale=float(w.view(torch.float32)[L.LS_SCALE]), growth_tracker=int(w[L.LS_GROWTH_TRACKER]),
                found_inf=int(w[L.LS_FOUND_INF]), steps=int(w[L.LS_ADAM_STEP]), skipped=int(w[L.LS_SKIPPED]))


# ----------------------------------------------------------------------------------------------------
# ops
# ----------------------------------------------------------------------------------------------------
def test_l1_scaled_bitwise_and_exact(ops):
    """B=2, 3 channels, 97x83, boundary_ignore 5 (a ragged last block on both paths: 16102 pixels)."""
    gen = torch.Generator().manual_seed(3)
    pred = (torch.rand(2, 3, 97, 83, generator=gen) - 0.2).to(DEV)          # some pixels behind the ReLU
    gt = torch.rand(2, 3, 97, 83, generator=gen).to(DEV)
    one = ops.loss_scale_state(1.0, DEV)
    # fp32 generic, fp16 with 8 channels (one 16-B store per pixel), fp16 generic (ld 16)
    for dt, ld in ((torch.float32, 8), (torch.float16, 8), (torch.float16, 16), (torch.bfloat16, 8)):
        l0, d0 = ops.l1_loss_backward(pred, gt, 5, dt, ld)
        l1, d1 = ops.l1_loss_backward(pred, gt, 5, dt, ld, state=one)
        assert torch.equal(_bits(l0), _bits(l1)), (dt, ld)
        assert torch.equal(_bits(d0), _bits(d1)), (dt, ld)
        assert float(d0.float().abs().max()) > 0
    l0, d0 = ops.l1_loss_backward(pred, gt, 5, torch.float32, 8)
    lk, dk = ops.l1_loss_backward(pred, gt, 5, torch.float32, 8, state=ops.loss_scale_state(2.0 ** 10, DEV))
    assert torch.equal(_bits(lk), _bits(l0))                                 # the loss is not scaled
    assert torch.equal(dk, d0 * 2.0 ** 10)
    # a product beyond fp16's range is stored as inf (visible to the overflow check), never saturated
    _, dh = ops.l1_loss_backward(pred, gt, 5, torch.float16, 8, state=ops.loss_scale_state(2.0 ** 40, DEV))
    assert bool(torch.isinf(dh).any()) and not bool(torch.isnan(dh).any())
    assert _state(one)['found_inf'] == 0 and _state(one)['scale'] == 1.0      # the op only reads the state


@pytest.mark.parametrize('n', [1, 7, 1025, 4099])
def test_unscale_check(ops, n):
    """Any n on a buffer that starts one float past a 16-B boundary: bitwise g * (1 / scale), nothing outside
    [0, n) touched, the flag 0; an inf at element 0 or a NaN at the last element sets it."""
    gen = torch.Generator().manual_seed(n)
    for scale in (65536.0, 3.0):
        host = torch.randn(n + 9, generator=gen) * 100.0
        buf = host.to(DEV)
        g = buf[1:1 + n]
        assert g.data_ptr() % 16 == 4
        st = ops.loss_scale_state(scale, DEV)
        ops.grad_unscale_check(g, st)
        inv = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(scale, dtype=torch.float32)
        ref = host.clone()
        ref[1:1 + n] = host[1:1 + n] * inv
        assert torch.equal(_bits(buf.cpu()), _bits(ref)), scale
        assert _state(st)['found_inf'] == 0
    for pos, bad in ((0, float('inf')), (n - 1, float('nan')), (n - 1, float('-inf'))):
        buf = torch.randn(n + 9, generator=gen).to(DEV)
        g = buf[1:1 + n]
        g[pos] = bad
        st = ops.loss_scale_state(65536.0, DEV)
        ops.grad_unscale_check(g, st)
        s = _state(st)
        assert s['found_inf'] == 1 and s['scale'] == 65536.0 and s['skipped'] == 0, (pos, bad)
    # a non-finite value just outside [0, n) is not this call's business
    buf = torch.randn(n + 9, generator=gen).to(DEV)
    buf[0], buf[n + 1] = float('nan'), float('inf')
    st = ops.loss_scale_state(2.0, DEV)
    ops.grad_unscale_check(buf[1:1 + n], st)
    assert _state(st)['found_inf'] == 0


def test_guarded_adam_and_update_sequence(ops):
    """[clean, clean, overflow, clean] with growth_interval 2: parameters and moments follow torch.optim.Adam
    stepped three times (test_train_step_adam_update_fp32's tolerance), the overflow step touches nothing and does
    not advance Adam's t, the state follows GradScaler's rule."""
    n = 4099
    gen = torch.Generator().manual_seed(5)
    p0 = torch.randn(n, generator=gen)
    grads = [torch.randn(n, generator=gen) * 0.1 for _ in range(4)]
    ref_p = p0.clone().requires_grad_()
    opt = torch.optim.Adam([ref_p], lr=1e-4)
    p, m, v = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    st = ops.loss_scale_state(8.0, DEV)
    expect = [dict(scale=8.0, growth_tracker=1, steps=1, skipped=0), dict(scale=16.0, growth_tracker=0, steps=2, skipped=0),
              dict(scale=8.0, growth_tracker=0, steps=2, skipped=1), dict(scale=8.0, growth_tracker=1, steps=3, skipped=1)]
    for i, g in enumerate(grads):
        scale = _state(st)['scale']
        gs = (g * scale).to(DEV)                      # what a backward from a scaled loss leaves (exact: 2^k)
        overflow = i == 2
        if overflow:
            gs[n // 2] = float('inf')
        before = [t.clone() for t in (p, m, v)]
        ops.grad_unscale_check(gs, st)
        ops.adam_step_guarded(p, gs, m, v, st, lr=1e-4)
        ops.loss_scale_update(st, 2.0, 0.5, 2)
        s = _state(st)
        assert s['found_inf'] == 0
        assert {k: s[k] for k in expect[i]} == expect[i], (i, s)
        if overflow:
            for a, b in zip((p, m, v), before):
                assert torch.equal(_bits(a), _bits(b))
            continue
        ref_p.grad = g.clone()
        opt.step()
        sd = opt.state[ref_p]
        for mine, ref in ((p, ref_p.detach()), (m, sd['exp_avg']), (v, sd['exp_avg_sq'])):
            np.testing.assert_allclose(mine.cpu().numpy(), ref.numpy(), rtol=1e-6, atol=1e-7)


# ----------------------------------------------------------------------------------------------------
# whole step
# ----------------------------------------------------------------------------------------------------
def _trainer(synth_sd, dtype, **kw):
    import dbsr_amd
    from dbsr_amd.training import DBSRTrainer
    net = dbsr_amd.dbsrnet_cvpr2021(**dbsr_amd.DBSR_SYNTHETIC_KWARGS)
    net.load_state_dict(synth_sd)
    net = net.to(DEV).set_compute_dtype(dtype)
    return net, DBSRTrainer(net, boundary_ignore=BI, **kw)


_CASES = {}


def _case(synth_sd, shape):
    """(burst, gt, oracle loss, oracle fp32 autograd gradients) of a shape, computed once."""
    if shape not in _CASES:
        from oracle import dbsr_oracle as orc
        from dbsr_amd.burst import synthetic_bursts
        B, N, H, W = shape
        burst, gt = synthetic_bursts(B, N, H, W, sr_factor=8, seed=17)
        sd = {k: v.clone().requires_grad_(not k.startswith('encoder.alignment_net')) for k, v in synth_sd.items()}
        pred, _ = orc.dbsr_forward(burst, sd)
        loss = F.l1_loss(pred[..., BI:-BI, BI:-BI], gt[..., BI:-BI, BI:-BI])
        loss.backward()
        _CASES[shape] = (burst, gt, float(loss.detach()), {k: v.grad for k, v in sd.items() if v.grad is not None})
    return _CASES[shape]


def _figures(mine, loss, ref_loss, ref_g):
    """(worst 1-cos, worst max-rel, loss relative error) over the parameter tensors, as test_train_step_grads_vs_oracle."""
    assert set(mine) == set(ref_g), set(mine) ^ set(ref_g)
    gmax = max(float(g.abs().max()) for g in ref_g.values())
    rel, cos = [], []
    for k, g in ref_g.items():
        if k == NOISE:
            assert float(mine[k].abs().max()) <= 1e-4 * gmax
            continue
        assert bool(torch.isfinite(mine[k]).all()), k
        rel.append((_rel(mine[k], g), k))
        cos.append((1 - float(F.cosine_similarity(mine[k].double().flatten(), g.double().flatten(), dim=0)), k))
    return max(cos), max(rel), abs(loss - ref_loss) / abs(ref_loss)


_BF16 = {}


def _bf16_figures(synth_sd, shape):
    """The bar: the existing bf16 trainer (no scaler) on the same inputs against the same oracle gradients."""
    if shape not in _BF16:
        burst, gt, ref_loss, ref_g = _case(synth_sd, shape)
        net, tr = _trainer(synth_sd, torch.bfloat16)
        assert tr.loss_scale_state() is None
        loss, _ = tr.forward_backward(burst.to(DEV), gt.to(DEV))
        torch.cuda.synchronize()
        _BF16[shape] = _figures({k: v.cpu() for k, v in tr.grads().items()}, float(loss), ref_loss, ref_g)
    return _BF16[shape]


def test_fp32_scaled_step_is_exact(synth_sd):
    """fp32, loss_scale=65536.0 against loss_scale=None: the same op list, gradients equal to 1e-7 of each tensor's
    max, one step's parameters equal to the Adam tolerance."""
    from dbsr_amd import _lib as L
    shape = (2, 3, 24, 32)
    burst, gt, _, _ = _case(synth_sd, shape)
    b, g = burst.to(DEV), gt.to(DEV)
    net0, tr0 = _trainer(synth_sd, torch.float32)
    net1, tr1 = _trainer(synth_sd, torch.float32, loss_scale=65536.0)
    assert tr0.loss_scale_state() is None and tr1.loss_scale_state()['scale'] == 65536.0
    l0, _ = tr0.forward_backward(b, g)
    l1, _ = tr1.forward_backward(b, g)
    torch.cuda.synchronize()
    assert not tr1.found_inf()
    assert float(l0) == float(l1)
    g0, g1 = tr0.grads(), tr1.grads()
    for k in g0:
        assert _rel(g1[k], g0[k]) <= 1e-7, (k, _rel(g1[k], g0[k]))
    # without loss_scale: today's ops under today's names; with it only the objective's launch differs
    ops0, ops1 = tr0.plans[shape].ops, tr1.plans[shape].ops
    assert [o[2] for o in ops0] == [o[2] for o in ops1]
    lib = L.lib()
    fe = tr0.plans[shape].fwd_end
    assert ops0[fe][2] == 'l1_loss_bwd' and ops0[fe][0] is lib.dbsr_l1_loss_backward
    assert ops1[fe][0] is lib.dbsr_l1_loss_backward_scaled
    assert all(a[0] is c[0] for i, (a, c) in enumerate(zip(ops0, ops1)) if i != fe)
    init = tr1.flat.detach().clone()
    tr0.step(b, g)
    tr1.step(b, g)
    torch.cuda.synchronize()
    np.testing.assert_allclose(tr1.flat.cpu().numpy(), tr0.flat.cpu().numpy(), rtol=1e-6, atol=1e-7)
    assert not torch.equal(tr1.flat, init)
    assert tr1.loss_scale_state() == dict(scale=65536.0, growth_tracker=1, steps=1, skipped=0)


@pytest.mark.parametrize('shape', [(2, 3, 24, 32), (1, 3, 48, 48), (1, 14, 24, 32)])
def test_fp16_grads_vs_oracle(synth_sd, shape):
    """fp16 with the default (dynamic, 65536) scaler against the oracle's fp32 autograd, the bf16 path as the bar.

    Measured on an MI355X, (worst 1-cos, worst max-rel, loss relative error), fp16 | bf16: DESIGN.md 'fp16 training'."""
    burst, gt, ref_loss, ref_g = _case(synth_sd, shape)
    bcos, brel, bloss = _bf16_figures(synth_sd, shape)
    net, tr = _trainer(synth_sd, torch.float16)
    assert tr.loss_scale_state() == dict(scale=65536.0, growth_tracker=0, steps=0, skipped=0)    # None -> 'dynamic'
    loss, _ = tr.forward_backward(burst.to(DEV), gt.to(DEV))
    torch.cuda.synchronize()
    if shape[1] == 14:
        assert 'wp.out+fuse' in [o[2] for o in tr.plans[shape].ops]            # the fused forward ran in fp16
    hcos, hrel, hloss = _figures({k: v.cpu() for k, v in tr.grads().items()}, float(loss), ref_loss, ref_g)
    print('shape', shape, 'loss', float(loss), ref_loss)
    print('fp16: 1-cos %.3e (%s)  max-rel %.3e (%s)  loss-rel %.3e' % (hcos + hrel + (hloss,)))
    print('bf16: 1-cos %.3e (%s)  max-rel %.3e (%s)  loss-rel %.3e' % (bcos + brel + (bloss,)))
    assert not tr.found_inf()                                  # no overflow at the initial scale
    assert tr.loss_scale_state() == dict(scale=65536.0, growth_tracker=0, steps=0, skipped=0)
    assert hcos[0] <= 3e-2 and hloss <= 1e-2, (hcos, hloss)     # bf16's bounds (test_train_step_grads_vs_oracle)
    assert hcos[0] <= bcos[0], (hcos, bcos)
    assert hrel[0] <= brel[0], (hrel, brel)
    assert hloss <= bloss, (hloss, bloss)


def test_overflow_step_is_skipped(synth_sd):
    """Scale 2^40: dP = 2^40 / count is inf in fp16 by construction, so the step's gradients are non-finite (no
    backward kernel forms an address from a gradient value: the warp gather bins by the forward flows).  The
    step leaves parameters and moments bitwise alone, counts a skip, halves the scale; the next step at 65536
    updates."""
    from dbsr_amd.burst import synthetic_bursts
    burst, gt = synthetic_bursts(1, 3, 24, 32, sr_factor=8, seed=19)
    b, g = burst.to(DEV), gt.to(DEV)
    net, tr = _trainer(synth_sd, torch.float16)
    tr.set_loss_scale(2.0 ** 40)
    before = [t.detach().clone() for t in (tr.flat, tr.exp_avg, tr.exp_avg_sq)]
    loss = tr.step(b, g)
    torch.cuda.synchronize()
    assert np.isfinite(float(loss))                            # the loss itself is not scaled
    for a, c in zip((tr.flat, tr.exp_avg, tr.exp_avg_sq), before):
        assert torch.equal(_bits(a), _bits(c))
    assert tr.loss_scale_state() == dict(scale=2.0 ** 39, growth_tracker=0, steps=0, skipped=1)
    tr.set_loss_scale(65536.0)
    tr.step(b, g)
    torch.cuda.synchronize()
    assert tr.loss_scale_state() == dict(scale=65536.0, growth_tracker=1, steps=1, skipped=1)
    assert not torch.equal(tr.flat, before[0])
    assert bool(torch.isfinite(tr.flat).all()) and bool(torch.isfinite(tr.exp_avg_sq).all())
    # Adam's first applied step has t = 1 although it is the trainer's second call: |dp| = lr |g| / (|g| + eps),
    # i.e. lr wherever the gradient is well above eps (t = 2 would give 0.74 lr); 2 % covers p's fp32 rounding
    big = tr.flat_grad.abs() > 1e-4
    assert bool(big.any())
    dp = (tr.flat - before[0]).abs()[big]
    assert float((dp - tr.lr).abs().max()) <= 2e-2 * tr.lr, (float(dp.min()), float(dp.max()))


def test_dynamic_run_over_graph_replays(synth_sd):
    burst, gt, _, _ = _case(synth_sd, (2, 3, 24, 32))
    b, g = burst.to(DEV), gt.to(DEV)
    net, tr = _trainer(synth_sd, torch.float16, growth_interval=2)
    losses = [float(tr.step(b, g)) for _ in range(4)]
    torch.cuda.synchronize()
    print('losses', losses)
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    assert tr.loss_scale_state() == dict(scale=4 * 65536.0, growth_tracker=0, steps=4, skipped=0)
    assert tr.plans[(2, 3, 24, 32)].graphs is not None
    assert bool(torch.isfinite(tr.flat).all())


def test_fixed_scale_skips_but_never_moves(synth_sd):
    """A float loss_scale: no growth, no backoff, an overflowing step is still skipped."""
    from dbsr_amd.burst import synthetic_bursts
    burst, gt = synthetic_bursts(1, 3, 24, 32, sr_factor=8, seed=19)
    b, g = burst.to(DEV), gt.to(DEV)
    net, tr = _trainer(synth_sd, torch.float16, loss_scale=2.0 ** 40, growth_interval=1)
    p0 = tr.flat.detach().clone()
    tr.step(b, g)
    assert tr.loss_scale_state() == dict(scale=2.0 ** 40, growth_tracker=0, steps=0, skipped=1)
    assert torch.equal(tr.flat, p0)
    tr.set_loss_scale(1024.0)
    tr.step(b, g)
    assert tr.loss_scale_state() == dict(scale=1024.0, growth_tracker=0, steps=1, skipped=1)
    assert not torch.equal(tr.flat, p0)


def test_autograd_fp16_under_gradscaler(synth_sd):
    """optimizer=False path: net.train() in fp16 under torch.amp.GradScaler + torch.optim.Adam, the reference loop.
    The trainer does not scale; the scaled upstream gradient keeps the fp16 backward in range."""
    import dbsr_amd
    shape = (2, 3, 24, 32)
    burst, gt, ref_loss, ref_g = _case(synth_sd, shape)
    bcos, brel, bloss = _bf16_figures(synth_sd, shape)
    b, g = burst.to(DEV), gt.to(DEV)
    net = dbsr_amd.dbsrnet_cvpr2021(**dbsr_amd.DBSR_SYNTHETIC_KWARGS)
    net.load_state_dict(synth_sd)
    net = net.to(DEV).set_compute_dtype(torch.float16).train()
    named = {k: p for k, p in net.named_parameters() if not k.startswith('encoder.alignment_net')}
    opt = torch.optim.Adam(list(named.values()), lr=1e-4)
    scaler = torch.amp.GradScaler('cuda')
    for it in range(2):
        opt.zero_grad()
        pred, _ = net(b)
        loss = F.l1_loss(pred[..., BI:-BI, BI:-BI], g[..., BI:-BI, BI:-BI])
        scaler.scale(loss).backward()
        scaler.unscale_(opt)
        if it == 0:
            assert net._train_engine.loss_scale_state() is None           # never scales internally
            mine = {k: p.grad.detach().cpu() for k, p in named.items()}
            hcos, hrel, hloss = _figures(mine, float(loss.detach()), ref_loss, ref_g)
            print('autograd fp16: 1-cos %.3e (%s)  max-rel %.3e (%s)  loss-rel %.3e' % (hcos + hrel + (hloss,)))
            assert hcos[0] <= 3e-2 and hloss <= 1e-2, (hcos, hloss)
            assert hcos[0] <= bcos[0] and hrel[0] <= brel[0] and hloss <= bloss, ((hcos, hrel, hloss), (bcos, brel, bloss))
        before = torch.cat([p.detach().reshape(-1).clone() for p in named.values()])
        scaler.step(opt)
        scaler.update()
        after = torch.cat([p.detach().reshape(-1) for p in named.values()])
        assert not torch.equal(before, after) and bool(torch.isfinite(after).all())
    assert scaler.get_scale() == 65536.0


def _ddp_worker(rank, world, port, sd_path, data_path, out_path):
    """One rank of a 2-process fp16 DBSRTrainer run over gloo, both ranks on cuda:0 (as test_gpu_train.py)."""
    import os
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        sd = torch.load(sd_path, weights_only=True)
        data = torch.load(data_path, weights_only=True)
        net, tr = _trainer(sd, torch.float16, growth_interval=2)
        assert tr.world == world
        b, g = data['burst'][rank:rank + 1].to(DEV), data['gt'][rank:rank + 1].to(DEV)
        losses = [float(tr.step(b, g)) for _ in range(2)]
        torch.cuda.synchronize()
        torch.save({'flat': tr.flat.cpu(), 'state': tr.loss_scale_state(), 'losses': losses}, out_path % rank)
    finally:
        dist.destroy_process_group()


def test_two_ranks_fp16_stay_in_sync(synth_sd, tmp_path):
    """world = 2, fp16, two steps (the second a graph replay): the all-reduce is a sum, so both ranks see the same
    summed gradients and take the same scaler decisions -- bitwise equal parameters, equal scaler state."""
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
    assert torch.equal(ranks[0]['flat'], ranks[1]['flat'])
    assert ranks[0]['state'] == ranks[1]['state'] == dict(scale=2 * 65536.0, growth_tracker=0, steps=2, skipped=0)
    assert bool(torch.isfinite(ranks[0]['flat']).all())
    assert all(np.isfinite(ranks[r]['losses']).all() for r in range(2))
