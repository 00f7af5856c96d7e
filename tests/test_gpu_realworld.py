"""The real-world fine-tuning objective on the HIP kernels (csrc/sca_train.hip): ops.aligned_l1, the autograd
SpatialColorAlignment, training.DBSRRealWorldTrainer -- against torch autograd of the same maths on the CPU
(tests/realworld_ref.py, which test_realworld_oracle.py pins to the reference's own loss and gradient).

Tolerances.  Op level, fp32 both sides with the flow, colour matrix and mask shared: the loss 1e-5 relative,
the gradient 1e-5 of its largest entry (at most 4 taps per contribution; the inputs keep |m - gt| >= 1e-2 so
no sign can flip on rounding).  Against the reference fixture the HIP flow differs from the reference's by up
to 1e-3 px (test_gpu_burstsr.py), which moves bilinear weights and flips a few signs: that bound is measured,
see test_sca_autograd_vs_reference_fixture.  The trainer's bars are test_gpu_train.py's."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


# ----------------------------------------------------------------------------------------------------
# ops.aligned_l1
# ----------------------------------------------------------------------------------------------------
def _flow(B, H, W, gen):
    """Random flow within +-3 px with the edge cases laid over it: a band sampled > 2 px above the image (all
    four taps in the zero padding), a band whose footprint is cut by the left edge, a block of integer flow and a
    block of exactly 0.5 px flow (bilinear weights 0 / 1 and 0.5)."""
    fl = (torch.rand(B, 2, H, W, generator=gen) - 0.5) * 6.0
    fl[:, 1, :3, :] = -6.0                                   # rows 0..2 sample y <= -3.5
    fl[:, 0, :, :2] = -1.3 - torch.arange(2.0)               # x + fx = -1.3: tap -2 (out) and -1 (out) / 0 (in)
    fl[:, 0, :, 2:4] = -2.6                                  # x + fx = -0.6 / 0.4: cut footprints
    fl[:, :, H // 2:H // 2 + 6, 4:12] = torch.tensor([2.0, -1.0]).view(1, 2, 1, 1)
    fl[:, :, H // 2 + 6:H // 2 + 12, 4:12] = torch.tensor([0.5, 1.5]).view(1, 2, 1, 1)
    return fl


def _case(shape, bi, seed, all_invalid=False):
    from tests.realworld_ref import aligned_l1
    B, _, H, W = shape
    gen = torch.Generator().manual_seed(seed)
    pred = torch.rand(B, 3, H, W, generator=gen)
    flow = _flow(B, H, W, gen)
    cmat = torch.eye(3).repeat(B, 1, 1) + 0.1 * torch.randn(B, 3, 3, generator=gen)
    valid = torch.rand(B, 1, H, W, generator=gen) < (0.0 if all_invalid else 0.7)
    # gt = the reference's colour-matched warp + an offset of 0.01 .. 0.1 with a random sign: |m - gt| >= 1e-2
    _, _, m = aligned_l1(pred, torch.zeros_like(pred), flow, cmat, valid, bi)
    off = (0.01 + 0.09 * torch.rand(B, 3, H, W, generator=gen)) * torch.sign(torch.rand(B, 3, H, W, generator=gen) - 0.5)
    gt = m + off
    ref_loss, ref_g, _ = aligned_l1(pred, gt, flow, cmat, valid, bi, weight=10.0)
    return pred, gt, flow, cmat, valid, ref_loss, ref_g


@pytest.mark.parametrize('shape,bi', [((1, 3, 33, 47), 0), ((1, 3, 33, 47), 8), ((2, 3, 128, 96), 40)])
def test_aligned_l1_vs_torch_autograd(shape, bi):
    from dbsr_amd import ops
    pred, gt, flow, cmat, valid, ref_loss, ref_g = _case(shape, bi, seed=shape[-1] + bi)
    args = [t.to(DEV) for t in (pred, gt, flow, cmat, valid)]
    loss, dpred = ops.aligned_l1(*args, bi, weight=10.0)
    loss2, _ = ops.aligned_l1(*args, bi, weight=10.0)
    print('loss', float(loss), float(ref_loss), 'dpred rel', _rel(dpred.cpu(), ref_g))
    assert torch.equal(loss, loss2)                                    # bitwise reproducible
    assert abs(float(loss) - float(ref_loss)) <= 1e-5 * abs(float(ref_loss))
    assert float(ref_g.abs().max()) > 0
    assert _rel(dpred.cpu(), ref_g) <= 1e-5


def test_aligned_l1_all_invalid():
    from dbsr_amd import ops
    pred, gt, flow, cmat, valid, ref_loss, ref_g = _case((2, 3, 33, 47), 8, seed=5, all_invalid=True)
    assert not valid.any() and float(ref_loss) == 0.0
    loss, dpred = ops.aligned_l1(*[t.to(DEV) for t in (pred, gt, flow, cmat, valid)], 8, weight=10.0)
    assert float(loss) == 0.0
    assert torch.count_nonzero(dpred).item() == 0 and bool(torch.isfinite(dpred).all())


@pytest.mark.parametrize('shape,bi', [((3, 3, 33, 47), 8), ((5, 3, 5, 7), 1)])
def test_aligned_l1_stats_per_image(shape, bi):
    """stats[b] = {masked squared-error sum, valid count} of image b inside the crop, from the loss's own pass:
    images whose pixel count is no multiple of the 256-pixel block (a block straddles two images) and images so
    small that one block spans all of them; PSNR(boundary_ignore) with the mask follows from them."""
    from dbsr_amd import ops
    from dbsr_amd.evaluation import PSNR
    from tests.realworld_ref import aligned_l1
    pred, gt, flow, cmat, valid, ref_loss, _ = _case(shape, bi, seed=21)
    _, _, m = aligned_l1(pred, gt, flow, cmat, valid, bi)
    loss2, _, stats = ops.aligned_l1_forward(*[t.to(DEV) for t in (pred, gt, flow, cmat, valid)], bi, 10.0)
    crop = (slice(None), slice(None), slice(bi, -bi), slice(bi, -bi))
    v = valid[crop].double()
    sq = (((m - gt)[crop].double() ** 2) * v).sum(dim=(1, 2, 3))
    st = stats.cpu().double()
    assert torch.equal(st[:, 1], v.sum(dim=(1, 2, 3))) and float(st[:, 1].min()) > 0
    assert float(((st[:, 0] - sq).abs() / sq).max()) <= 1e-5
    assert abs(float(loss2[0]) - float(ref_loss)) <= 1e-5 * float(ref_loss)
    psnr = float(PSNR(boundary_ignore=bi)(m, gt, valid=valid))
    mine = float((-10.0 * torch.log10(st[:, 0] / (3.0 * st[:, 1] + 1e-12))).mean())
    assert abs(mine - psnr) <= 1e-3, (mine, psnr)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_aligned_l1_null_alignment_is_the_l1_objective(dtype):
    """flow = c_mat = valid = NULL, weight 1: the loss and the predictor's gated gradient dP of
    dbsr_l1_loss_backward -- dP exactly; the loss bitwise where that op sums in 256-pixel blocks (fp32 dP; its
    16-bit path sums 1024 pixels per block, another fp32 order: 4e-6 relative there)."""
    from dbsr_amd import _lib as L
    from dbsr_amd import ops
    B, H, W, bi = 2, 56, 72, 8
    gen = torch.Generator().manual_seed(3)
    pred = F.relu(torch.randn(B, 3, H, W, generator=gen)).to(DEV)      # zeros: the ReLU gate is exercised
    gt = torch.rand(B, 3, H, W, generator=gen).to(DEV)
    dP = torch.zeros(B, H, W, 8, dtype=dtype, device=DEV)
    loss = torch.zeros(1, device=DEV)
    nlb = (B * H * W + 255) // 256
    ws = torch.zeros(nlb, device=DEV)
    L.check(L.lib().dbsr_l1_loss_backward(B, 3, H, W, bi, pred.data_ptr(), gt.data_ptr(), L.tensor_desc(dP, 8),
                                          loss.data_ptr(), ws.data_ptr(), 4 * nlb, L.stream_ptr(pred.device)), 'l1')
    loss2, g, _ = ops.aligned_l1_forward(pred, gt, None, None, None, bi, 1.0)
    gpred, mine = ops.aligned_l1_backward(g, None, pred=pred, scale=loss2[1:], dpre_dtype=dtype)
    assert torch.count_nonzero(dP).item() > 0
    assert torch.equal(mine, dP)
    if dtype == torch.float32:
        assert torch.equal(loss2[:1], loss)
    else:
        # each side adds every term along a path of at most ~30 fp32 additions: 2 x 30 x 2^-24
        assert abs(float(loss2[0]) - float(loss)) <= 4e-6 * float(loss)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_gated_nhwc_output_is_relu_grad_of_gpred(dtype):
    """One launch writes both layouts: the NHWC dP equals dbsr_relu_grad of the fp32 NCHW gpred, exactly."""
    from dbsr_amd import _lib as L
    from dbsr_amd import ops
    pred, gt, flow, cmat, valid, _, _ = _case((2, 3, 40, 56), 8, seed=9)
    pred = F.relu(pred - 0.3)                                            # a third of the prediction gated off
    pred, gt, flow, cmat, valid = (t.to(DEV) for t in (pred, gt, flow, cmat, valid))
    loss2, g, _ = ops.aligned_l1_forward(pred, gt, flow, cmat, valid, 8, 10.0)
    gpred, dP = ops.aligned_l1_backward(g, flow, pred=pred, scale=loss2[1:], dpre_dtype=dtype)
    ref = torch.zeros_like(dP)
    L.check(L.lib().dbsr_relu_grad(2, 3, 40, 56, pred.data_ptr(), gpred.data_ptr(), L.tensor_desc(ref, 8),
                                   L.stream_ptr(pred.device)), 'relu_grad')
    assert torch.count_nonzero(ref).item() > 0 and torch.count_nonzero(ref[..., 3:]).item() == 0
    assert torch.equal(dP, ref)


# ----------------------------------------------------------------------------------------------------
# autograd SpatialColorAlignment
# ----------------------------------------------------------------------------------------------------
def _pwc(synth_sd):
    from dbsr_amd.pwcnet import PWCNet
    pre = 'encoder.alignment_net.'
    net = PWCNet(load_pretrained=False)
    net.load_state_dict({k[len(pre):]: v for k, v in synth_sd.items() if k.startswith(pre)})
    return net.to(DEV)


# measured on MI355X (see the docstring below); the assertion is 3x this, never looser than 2e-2
SCA_FIXTURE_GRAD_MEASURED = 1.2e-5


def test_sca_autograd_vs_reference_fixture(golden, synth_sd):
    """The reference's loop on fixture A: out, valid = sca(pred, gt, burst); (10 * obj(out, gt, valid=valid))
    .backward().  Forward outputs meet test_gpu_burstsr.py's fixture bars; pred.grad is compared with the
    reference's (realworld.npz) on the pixels where the two validity masks agree, at most 1 % of the pixels
    left out; with the flow, C and mask shared (torch autograd from last_alignment) it must match to 1e-5.

    Measured on MI355X (fp32 PWC engine): the two masks agree everywhere (0 % left out); max |grad - reference| /
    max |reference| = 1.20e-5 (the HIP flow is within 1e-3 px of the reference's, which moves the bilinear
    weights); with the alignment shared 1.95e-7.  Asserted: 3 x 1.2e-5 = 3.6e-5."""
    from dbsr_amd import burstsr as bs
    from tests.realworld_ref import aligned_l1
    g, r = golden('burstsr'), golden('realworld')
    sca = bs.SpatialColorAlignment(_pwc(synth_sd), sr_factor=4)
    obj = bs.PixelWiseError(metric='l1', boundary_ignore=40)
    pred = torch.from_numpy(g['a_pred']).to(DEV).requires_grad_(True)
    gt, burst = torch.from_numpy(g['a_gt']).to(DEV), torch.from_numpy(g['a_burst']).to(DEV)
    out, valid = sca(pred, gt, burst)
    assert out.requires_grad and not valid.requires_grad
    loss = 10 * obj(out, gt, valid=valid)
    loss.backward()
    flow, cmat, valid2 = sca.last_alignment
    assert torch.equal(valid, valid2)
    # forward: the existing fixture bars
    assert (flow.cpu() - torch.from_numpy(g['a_flow'])).abs().max().item() <= 1e-3
    np.testing.assert_allclose(cmat.cpu().numpy(), g['a_cmat'], rtol=2e-3, atol=2e-3)
    v = valid.cpu().numpy()
    assert (v == g['a_valid']).mean() >= 0.99
    both = v & g['a_valid']
    d = np.abs(out.detach().cpu().numpy() - g['a_out'])[np.broadcast_to(both, g['a_out'].shape)]
    assert d.max() <= 5e-3, d.max()
    print('loss', float(loss.detach()), float(r['loss']))
    # gradient, flow / C / mask shared: torch autograd from last_alignment
    _, ref_g, _ = aligned_l1(torch.from_numpy(g['a_pred']), gt.cpu(), flow.cpu(), cmat.cpu(), valid.cpu(), 40, 10.0)
    mine = pred.grad.cpu()
    shared = _rel(mine, ref_g)
    print('grad vs torch with the shared alignment: max diff / max', shared)
    assert shared <= 1e-5
    # gradient vs the reference's own, on the pixels where the two masks agree
    agree = torch.from_numpy(v == g['a_valid'])
    assert float((~agree).float().mean()) <= 0.01
    ref = torch.from_numpy(r['dpred'])
    meas = float(((mine - ref).abs() * agree).max() / ref.abs().max())
    print('grad vs the reference fixture: max diff / max', meas, 'left out', float((~agree).float().mean()))
    bound = min(2e-2, 3 * SCA_FIXTURE_GRAD_MEASURED)
    assert meas <= bound, (meas, bound)


# ----------------------------------------------------------------------------------------------------
# DBSRRealWorldTrainer
# ----------------------------------------------------------------------------------------------------
def _net(synth_sd, dtype):
    import dbsr_amd
    net = dbsr_amd.dbsrnet_cvpr2021(**dbsr_amd.DBSR_SYNTHETIC_KWARGS)
    net.load_state_dict(synth_sd)
    return net.to(DEV).set_compute_dtype(dtype)


def _rw_trainer(synth_sd, dtype):
    from dbsr_amd.training import DBSRRealWorldTrainer
    net = _net(synth_sd, dtype)
    return net, DBSRRealWorldTrainer(net, _pwc(synth_sd), sr_factor=4, loss_weight=10.0, boundary_ignore=40)


@pytest.fixture(scope='module')
def fp32_step(synth_sd):
    """One fp32 forward_backward on a (1, 3, 16, 16) burst (a 128 x 128 prediction), shared by the tests below:
    (burst, gt, loss, gradients, last_alignment, last_stats, prediction), all on the CPU."""
    from dbsr_amd.burst import synthetic_bursts
    burst, gt = synthetic_bursts(1, 3, 16, 16, sr_factor=8, seed=17)
    net, tr = _rw_trainer(synth_sd, torch.float32)
    loss, pred = tr.forward_backward(burst.to(DEV), gt.to(DEV))
    torch.cuda.synchronize()
    return dict(burst=burst, gt=gt, loss=float(loss), grads={k: v.cpu().clone() for k, v in tr.grads().items()},
                align=tuple(t.cpu() for t in tr.last_alignment), stats=tr.last_stats, pred=pred.cpu().clone())


# measured on MI355X: |fused loss - loss with the oracle's own alignment| / loss (see the docstring below)
TRAINER_OWN_ALIGNMENT_LOSS_MEASURED = 0.0


def test_realworld_trainer_grads_vs_oracle(synth_sd, fp32_step):
    """Loss and every parameter gradient against oracle autograd (oracle.dbsr_forward -> warp -> C -> masked L1
    x 10) with the trainer's own flow / C / mask: test_train_step_grads_vs_oracle's fp32 bars (loss 1e-5,
    per-tensor 1 - cos <= 1e-4, max-rel <= 2e-2).  With the oracle's own alignment (its PWC flow from its own
    prediction) the loss moves by the measured amount below.

    Measured on MI355X: fused loss 5.704160690 against 5.704161167 with the shared alignment (8e-8 relative) and
    5.704160690 with the oracle's own alignment: the difference is 0.0 in fp32 (the mask is the same, the flows
    differ by < 1e-3 px on a smooth image).  3 x 0 is no bound a float can keep, so the assertion is the fp32
    loss bar the shared-alignment comparison already uses, 1e-5, which the own-alignment difference cannot
    undercut (it contains that comparison's rounding)."""
    from oracle import dbsr_oracle as orc
    from tests.realworld_ref import masked_l1, sca_objective
    s = fp32_step
    flow, cmat, valid = s['align']
    assert 0.2 < float(valid[..., 40:-40, 40:-40].float().mean()) < 0.95
    sd = {k: v.clone().requires_grad_(not k.startswith('encoder.alignment_net')) for k, v in synth_sd.items()}
    pred, _ = orc.dbsr_forward(s['burst'], sd)
    m = torch.einsum('bchw,bck->bkhw', orc.warp(pred, flow), cmat)
    ref_loss = masked_l1(m, s['gt'], valid.bool(), 40, 10.0)
    ref_loss.backward()
    ref_loss = ref_loss.detach()
    ref_g = {k: v.grad for k, v in sd.items() if v.grad is not None}
    mine = s['grads']
    assert set(mine) == set(ref_g), set(mine) ^ set(ref_g)
    print('loss', s['loss'], float(ref_loss))
    assert abs(s['loss'] - float(ref_loss)) <= 1e-5 * max(1.0, abs(float(ref_loss)))
    gmax = max(float(g.abs().max()) for g in ref_g.values())
    rel, cos = [], []
    for k, g in ref_g.items():
        if k == 'merging.weight_predictor.4.0.bias':
            # shared by all N frames of the softmax: its exact gradient is 0 (as test_train_step_grads_vs_oracle)
            assert float(mine[k].abs().max()) <= 1e-4 * gmax
            continue
        rel.append((_rel(mine[k], g), k))
        cos.append((1 - float(F.cosine_similarity(mine[k].double().flatten(), g.double().flatten(), dim=0)), k))
    rel.sort(reverse=True)
    cos.sort(reverse=True)
    print('max-rel worst', rel[:4])
    print('1-cos worst', cos[:4])
    assert rel[0][0] <= 2e-2, rel[:3]
    assert cos[0][0] <= 1e-4, cos[:3]
    # the actor's statistics: Loss/total and Stat/psnr (PSNR(boundary_ignore=40) with the mask)
    from dbsr_amd.evaluation import PSNR
    psnr = float(PSNR(boundary_ignore=40)(m.detach(), s['gt'], valid=valid.bool()))
    print('psnr', s['stats']['psnr'], psnr)
    assert abs(s['stats']['loss'] - s['loss']) == 0 and abs(s['stats']['psnr'] - psnr) <= 1e-3
    # the oracle's own alignment
    own_loss, _, _ = sca_objective(pred.detach(), s['gt'], s['burst'], synth_sd, bi=40, weight=10.0)
    meas = abs(s['loss'] - float(own_loss)) / float(own_loss)
    print('loss with the oracle\'s own alignment', float(own_loss), 'relative difference', meas)
    bound = max(3 * TRAINER_OWN_ALIGNMENT_LOSS_MEASURED, 1e-5)
    assert meas <= bound, (meas, bound)


def test_fused_step_matches_autograd_loop(synth_sd, fp32_step):
    """The reference-style loop on the same weights -- net(burst) in train mode, the autograd
    SpatialColorAlignment, PixelWiseError, backward() -- gives the fused step's loss (1e-6 relative) and gradients
    (1e-5 of each tensor's largest entry; the objective's scatter-add is not bitwise reproducible)."""
    from dbsr_amd import burstsr as bs
    s = fp32_step
    net = _net(synth_sd, torch.float32).train()
    sca = bs.SpatialColorAlignment(_pwc(synth_sd), sr_factor=4)
    obj = bs.PixelWiseError(metric='l1', boundary_ignore=40)
    burst, gt = s['burst'].to(DEV), s['gt'].to(DEV)
    pred, _ = net(burst)
    out, valid = sca(pred, gt, burst)
    loss = 10 * obj(out, gt, valid=valid)
    loss.backward()
    torch.cuda.synchronize()
    print('loss', float(loss), s['loss'])
    assert abs(float(loss) - s['loss']) <= 1e-6 * s['loss']
    grads = {k: p.grad.cpu() for k, p in net.named_parameters() if p.grad is not None}
    assert set(grads) == set(s['grads'])
    gmax = max(float(g.abs().max()) for g in s['grads'].values())
    zero_bias = 'merging.weight_predictor.4.0.bias'       # exact gradient 0 (softmax shift invariance): noise
    assert float((grads[zero_bias] - s['grads'][zero_bias]).abs().max()) <= 1e-5 * gmax
    worst = max((_rel(grads[k], g), k) for k, g in s['grads'].items() if k != zero_bias)
    print('worst gradient difference / max', worst)
    assert worst[0] <= 1e-5, worst


def test_realworld_step_bf16(synth_sd, fp32_step):
    """bf16 step() twice (the second replays the captured graphs) on a (2, 3, 16, 16) burst: the loss finite
    and within 1 % of the fp32 trainer's (the bf16 bar of test_gpu_train.py), parameters change, the inference
    engine is told its packed weights are stale."""
    from dbsr_amd.burst import synthetic_bursts
    burst, gt = synthetic_bursts(2, 3, 16, 16, sr_factor=8, seed=17)
    burst, gt = burst.to(DEV), gt.to(DEV)
    _, tr32 = _rw_trainer(synth_sd, torch.float32)
    ref_loss, _ = tr32.forward_backward(burst, gt)
    ref_loss = float(ref_loss)
    net, tr = _rw_trainer(synth_sd, torch.bfloat16)
    with torch.no_grad():
        net.eval()(burst)                                    # builds the inference engine the step must flag
    net._engine.weights_stale = False
    before = tr.flat.clone()
    l1 = float(tr.step(burst, gt))
    assert net._engine.weights_stale
    mid = tr.flat.clone()
    l2 = float(tr.step(burst, gt))
    torch.cuda.synchronize()
    plan = next(iter(tr.plans.values()))
    assert plan.graphs is not None                           # the second step replayed graphs
    print('bf16 losses', l1, l2, 'fp32', ref_loss)
    assert np.isfinite(l1) and np.isfinite(l2)
    assert abs(l1 - ref_loss) <= 1e-2 * ref_loss
    assert not torch.equal(before, mid) and not torch.equal(mid, tr.flat)
    assert bool(torch.isfinite(tr.flat).all())
    st = tr.last_stats
    assert np.isfinite(st['psnr']) and st['loss'] == l2


def test_realworld_trainer_refuses_fp16(synth_sd):
    from dbsr_amd.training import DBSRRealWorldTrainer
    with pytest.raises(ValueError, match='bfloat16'):
        DBSRRealWorldTrainer(_net(synth_sd, torch.float16), _pwc(synth_sd))
