"""Training PWC-Net end to end: the differentiable forward of pwcnet.PWCNet (torch.ops.dbsr.* with HIP backwards),
DBSRNet.forward with train_alignmentnet=True, and DBSRTrainer(alignment_grad=True), against float64 autograd through
the oracle on the CPU.  Bars: the project's fp32 bars (test_trainer_flow_grad_vs_oracle): flow within 1e-4 of its
max, 1 - cos <= 1e-4 over the flat gradient, per-tensor max|d| / max|ref| <= 2e-2.

The input is synthetic_bursts(1, 3, 24, 32, sr_factor=8, seed=5): the oracle alone is stable on it (fp32 against
float64 on the CPU: no LeakyReLU sign, mask threshold or bilinear cell flips); (1, 3, 48, 48) is not."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = 'cuda'
B, N, H, W = 1, 3, 24, 32
SEED = 5
PWC = 'encoder.alignment_net.'


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-300))


def _cos(a, b):
    return 1 - float(F.cosine_similarity(a.double().flatten(), b.double().flatten(), dim=0))


def _net(synth_sd, train_alignmentnet=True):
    import dbsr_amd
    net = dbsr_amd.dbsrnet_cvpr2021(**dict(dbsr_amd.DBSR_SYNTHETIC_KWARGS, train_alignmentnet=train_alignmentnet))
    net.load_state_dict(synth_sd)
    return net.to(DEV)


def _rgb_pairs(burst):
    x_rgb = torch.stack((burst[:, :, 0], burst[:, :, 1:3].mean(dim=2), burst[:, :, 3]), dim=2)
    x_ref = x_rgb[:, :1].repeat(1, burst.shape[1] - 1, 1, 1, 1).contiguous()
    x_oth = x_rgb[:, 1:].contiguous()
    return x_oth.view(-1, *x_oth.shape[-3:]), x_ref.view(-1, *x_ref.shape[-3:])


@pytest.fixture(scope='module')
def case():
    from dbsr_amd.burst import synthetic_bursts
    burst, gt = synthetic_bursts(B, N, H, W, sr_factor=8, seed=SEED)
    return dict(burst=burst, gt=gt)


def _compare(mine, ref, what):
    """mine / ref: {name: gradient} over the same PWC tensors; prints, then applies the fp32 bars."""
    assert set(mine) == set(ref) and len(ref) == 126, (len(mine), len(ref))
    keys = sorted(ref)
    cos = _cos(torch.cat([mine[k].flatten() for k in keys]), torch.cat([ref[k].flatten() for k in keys]))
    rel = sorted(((_rel(mine[k], ref[k]), k) for k in keys), reverse=True)
    print('%s: 126 tensors, 1-cos %.3g, worst per-tensor max-rel %s' % (what, cos, rel[:3]))
    assert cos <= 1e-4, cos
    assert rel[0][0] <= 2e-2, rel[:3]


def test_pwc_parameter_gradients_vs_oracle(synth_sd, case):
    """The 126 PWC-Net parameter gradients of loss = (flow * G).sum() in fp32 against oracle.pwcnet under float64
    autograd.  Checked on the CPU, the oracle in fp32 against float64 on this input gives 1 - cos = 1e-13 and a worst
    per-tensor max-rel of 2.5e-6."""
    from oracle import dbsr_oracle as orc
    src, tgt = _rgb_pairs(case['burst'])
    G = torch.randn(B * (N - 1), 2, H, W, generator=torch.Generator().manual_seed(1))
    sd = {k: v.double().clone().requires_grad_(k.startswith(PWC)) for k, v in synth_sd.items()}
    ref_flow = orc.pwcnet(src.double(), tgt.double(), sd)
    (ref_flow * G.double()).sum().backward()
    ref = {k: v.grad for k, v in sd.items() if v.grad is not None}
    net = _net(synth_sd).train()
    pwc = net.encoder.alignment_net
    assert pwc.differentiable is True
    flow = pwc(src.to(DEV), tgt.to(DEV))
    assert flow.grad_fn is not None and flow.shape == (B * (N - 1), 2, H, W) and flow.dtype == torch.float32
    ferr = float((flow.detach().cpu().double() - ref_flow.detach()).abs().max())
    fmax = float(ref_flow.detach().abs().max())
    print('differentiable PWC flow: max |err| %.3g of max |flow| %.3g' % (ferr, fmax))
    assert ferr <= 1e-4 * fmax
    (flow * G.to(DEV)).sum().backward()
    mine = {PWC + k: p.grad.cpu() for k, p in pwc.named_parameters() if p.grad is not None}
    _compare(mine, ref, 'PWC gradients of (flow * G).sum()')


def test_whole_net_backward_fills_all_231_gradients(synth_sd, case):
    """dbsrnet_cvpr2021(train_alignmentnet=True) in fp32 with the L1 loss: loss.backward() gives a finite .grad on
    all 231 tensors, and the PWC gradients match oracle.dbsr_forward under float64 autograd at the same bars.  Seed 5
    was checked first: the oracle's 126 PWC gradients in fp32 against float64 on the CPU give |1 - cos| < 1e-13 and a
    worst per-tensor max-rel of 1.7e-6 (netExtractor.netOne.0.weight), under one tenth of each bar, so seed 5 it is."""
    from oracle import dbsr_oracle as orc
    burst, gt = case['burst'], case['gt']
    sd = {k: v.double().clone().requires_grad_(True) for k, v in synth_sd.items()}
    pred64, _ = orc.dbsr_forward(burst.double(), sd)
    F.l1_loss(pred64, gt.double()).backward()
    ref = {k: v.grad for k, v in sd.items() if k.startswith(PWC) and v.grad is not None}
    net = _net(synth_sd).train()
    pred, aux = net(burst.to(DEV))
    assert pred.grad_fn is not None and aux['offsets'].shape == (B, N - 1, 2, H, W)
    perr = float((pred.detach().cpu().double() - pred64.detach()).abs().max())
    print('pred max |err| %.3g' % perr)
    F.l1_loss(pred, gt.to(DEV)).backward()
    named = dict(net.named_parameters())
    assert len(named) == 231
    missing = [k for k, p in named.items() if p.grad is None or not bool(torch.isfinite(p.grad).all())]
    assert not missing, missing
    _compare({k: named[k].grad.cpu() for k in ref}, ref, 'PWC gradients of the L1 loss through the whole net')


def test_trainer_alignment_grad_step(synth_sd, case):
    """One DBSRTrainer(alignment_grad=True) step: the PWC gradients are the autograd path's (the bar of
    test_autograd_trains_an_alignment_module), every PWC parameter with a nonzero gradient moved against its sign by
    at most 1.01 lr (Adam's first step), and the DBSR parameters take the update of a step given the same flow."""
    from dbsr_amd.dbsrnet import alignment_flow
    from dbsr_amd.training import DBSRTrainer
    lr = 1e-4
    b, g = case['burst'].to(DEV), case['gt'].to(DEV)
    # the autograd path, for the gradients and the flow
    net_a = _net(synth_sd).train()
    pred, _ = net_a(b)
    F.l1_loss(pred, g).backward()
    auto = {k: p.grad.clone() for k, p in net_a.named_parameters() if k.startswith(PWC)}
    flow = alignment_flow(net_a, b).detach()
    # the trainer
    net_t = _net(synth_sd).train()
    before = {k: p.detach().clone() for k, p in net_t.named_parameters()}
    tr = DBSRTrainer(net_t, lr=lr, boundary_ignore=0, alignment_grad=True)
    loss = tr.step(b, g)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss).all())
    named = dict(net_t.named_parameters())
    moved = 0
    for k, p in named.items():
        if not k.startswith(PWC):
            continue
        gr = tr.pwc_grad_view(p)
        torch.testing.assert_close(gr, auto[k], rtol=1e-4, atol=1e-6 * float(auto[k].abs().max()), msg=lambda m: k + ': ' + m)
        delta = p.detach() - before[k]
        nz = gr != 0
        assert float(delta.abs().max()) <= 1.01 * lr, k
        assert bool((delta[nz] * gr[nz] <= 0).all()), k
        assert bool((delta[~nz] == 0).all()), k
        moved += int((delta[nz] != 0).sum())
    assert moved > 0
    # the DBSR parameters: the same update as a step with that flow passed in
    net_f = _net(synth_sd, train_alignmentnet=False).train()
    tf = DBSRTrainer(net_f, lr=lr, boundary_ignore=0)
    tf.step(b, g, flow=flow)
    torch.cuda.synchronize()
    other = dict(net_f.named_parameters())
    for k, p in named.items():
        if not k.startswith(PWC):
            assert torch.equal(p.detach(), other[k].detach()), k


def test_refused_combinations(synth_sd):
    from dbsr_amd.training import DBSRTrainer
    net = _net(synth_sd)
    with pytest.raises(NotImplementedError, match='train_alignmentnet'):
        DBSRTrainer(net)
    with pytest.raises(NotImplementedError, match='loss_scale with alignment_grad'):
        DBSRTrainer(net, alignment_grad=True, loss_scale='dynamic')
    with pytest.raises(NotImplementedError, match='loss_scale with alignment_grad'):
        DBSRTrainer(net.set_compute_dtype(torch.float16), alignment_grad=True)       # fp16 means 'dynamic'
    net.set_compute_dtype(torch.float32)
    import torch.distributed as dist                 # the refusal itself, without a process group
    real = (dist.is_available, dist.is_initialized, dist.get_world_size)
    dist.is_available, dist.is_initialized, dist.get_world_size = (lambda: True), (lambda: True), (lambda *a, **k: 2)
    try:
        with pytest.raises(NotImplementedError, match='world size > 1 with alignment_grad'):
            DBSRTrainer(net, alignment_grad=True)
    finally:
        dist.is_available, dist.is_initialized, dist.get_world_size = real


def test_non_differentiable_forward_is_the_engine(synth_sd, case):
    """differentiable=False (the default): PWCNet.forward in train mode is today's engine path -- no grad_fn, and
    bitwise the eval-mode engine output."""
    net = _net(synth_sd, train_alignmentnet=False)
    pwc = net.encoder.alignment_net
    assert pwc.differentiable is False
    src, tgt = _rgb_pairs(case['burst'])
    src, tgt = src.to(DEV), tgt.to(DEV)
    pwc.train()
    a = pwc(src, tgt)
    assert a.grad_fn is None and not a.requires_grad
    pwc.eval()
    with torch.no_grad():
        bb = pwc(src, tgt)
    assert torch.equal(a, bb)
