"""Training step of the DBSR network on the HIP kernels (BASELINE.json configs[3]; SURVEY §8e training
row, §8f rank 3).

The reference step (trainers/simple_trainer.py:78-81 with actors/dbsr_actors.py:27-47 and the
train_settings/dbsr/default_synthetic.py:85-96 objective / optimizer):

    pred, _ = net(burst); loss = L1(pred, frame_gt, boundary_ignore=40)
    optimizer.zero_grad(); loss.backward(); optimizer.step()        # Adam, lr 1e-4

PWC-Net is frozen (train_alignmentnet=False: its forward runs under no_grad, encoders.py:56-61), so
only the 3.64 M DBSR parameters train.  Multi-GPU: the reference wraps the net in nn.DataParallel
(admin/multigpu.py:8-14); here one process per GPU runs its shard of the global batch and the fp32
gradients are averaged by bucketed RCCL all-reduces (torch.distributed) that start as soon as the
backward of a bucket's layers has been issued, overlapping the rest of the backward.

Every op of the step is a C-ABI launch (libdbsr_hip.so): the forward reuses the inference plan's
kernels with every saved activation in its own buffer, conv dgrad is dbsr_conv2d on dgrad-packed
weights with the gate/residual epilogue (ReLU and ResBlock backward fused into the conv), conv wgrad
is dbsr_conv_wgrad (MFMA), and the remaining backward ops and Adam are the train_ops kernels.
"""
import ctypes
import math

import torch
import torch.distributed as dist

from . import _lib as L
from ._lib import IDENTITY
from .engine import NHWC, Plan, PWCPlanner, _Weights, cpad, gauss_kernel3, merging_variant, r8


class _WS:
    """Placeholder for a scratch pointer patched in once the plan knows its largest request."""
    def __init__(self, kind, nbytes):
        self.kind, self.nbytes = kind, int(nbytes)


class PackedW:
    """Packed MFMA weights built from a fp32 torch-layout weight tensor (re-packed after every update)."""
    def __init__(self, w, b, dtype, device, shuffle=1, stride=1, pad=None, dil=1):
        self.src_w, self.src_b = w, b
        self.cout, self.cin, self.kh, self.kw = w.shape
        self.stride, self.dil = stride, dil
        self.pad = self.kh // 2 if pad is None else pad
        self.shuffle = shuffle
        self.dtype = dtype
        self.w = torch.empty(L.lib().dbsr_conv_packed_elems(self.cout, self.cin, self.kh, self.kw), dtype=dtype,
                             device=device)
        self.bias = torch.empty(self.cout, dtype=torch.float32, device=device) if b is not None else None

    def out_hw(self, h, w):
        return ((h + 2 * self.pad - self.dil * (self.kh - 1) - 1) // self.stride + 1,
                (w + 2 * self.pad - self.dil * (self.kw - 1) - 1) // self.stride + 1)

    def pack_args(self):
        return (self.src_w.data_ptr(), self.src_b.data_ptr() if self.src_b is not None else None, self.cout, self.cin,
                self.kh, self.kw, L.dtype_code(self.dtype), self.shuffle, self.w.data_ptr(),
                self.bias.data_ptr() if self.bias is not None else None)


class TConv:
    """A trainable nn.Conv2d: forward-packed weights, dgrad weights (transposed + flipped, packed), and
    where its gradients live in the flat gradient buffer."""
    def __init__(self, mod, trainer, dtype, device, shuffle=1):
        self.mod = mod
        w, b = mod.weight, mod.bias
        self.fwd = PackedW(w.data, b.data if b is not None else None, dtype, device, shuffle=shuffle)
        co, ci, kh, kw = w.shape
        self.wt = torch.empty(ci, co, kh, kw, dtype=torch.float32, device=device)
        self.bwd = PackedW(self.wt, None, dtype, device)
        self.gw = trainer.grad_view(w)
        self.gb = trainer.grad_view(b) if b is not None else None
        self.cout, self.cin, self.k = co, ci, kh

    def sub_dgrad(self, lo, hi, dtype, device):
        """dgrad weights producing only input channels [lo, hi) (a slice of wt: rows of the dgrad conv)."""
        p = PackedW(self.wt[lo:hi], None, dtype, device)
        self.extra = getattr(self, 'extra', []) + [p]
        return p

    def pack_jobs(self):
        """This conv's repacks as dbsr_pack_job entries (dbsr_conv_pack_weights_batch): the forward weights and
        every dgrad copy, the latter straight from the module's weight (no fp32 transpose pass)."""
        code = L.dtype_code(self.fwd.dtype)
        w = self.mod.weight
        f = self.fwd
        jobs = [L.PackJob(w=w.data_ptr(), bias=f.src_b.data_ptr() if f.src_b is not None else None,
                          w_packed=f.w.data_ptr(), bias_out=f.bias.data_ptr() if f.bias is not None else None,
                          cout=f.cout, cin=f.cin, kh=f.kh, kw=f.kw, dtype=code, shuffle=f.shuffle)]
        for p in [self.bwd] + getattr(self, 'extra', []):
            # p packs rows [lo, lo + p.cout) of wt = w transposed (ci, co) and flipped
            lo = (p.src_w.data_ptr() - self.wt.data_ptr()) // (4 * self.cout * self.k * self.k)
            jobs.append(L.PackJob(w=w.data_ptr(), bias=None, w_packed=p.w.data_ptr(),
                                  bias_out=p.bias.data_ptr() if p.bias is not None else None, cout=p.cout, cin=p.cin,
                                  kh=p.kh, kw=p.kw, dtype=code, shuffle=1, transposed=1, lo=lo, src_cin=self.cin))
        return jobs

    def repack_ops(self, plan):
        lib = L.lib()
        plan.add('pack.' + self.name, lib.dbsr_conv_pack_weights, *self.fwd.pack_args())
        w = self.mod.weight
        plan.add('dgradw.' + self.name, lib.dbsr_dgrad_weights, w.data_ptr(), self.cout, self.cin, self.k, self.k,
                 self.wt.data_ptr())
        for p in [self.bwd] + getattr(self, 'extra', []):
            plan.add('packT.' + self.name, lib.dbsr_conv_pack_weights, *p.pack_args())


class DBSRTrainer:
    """One optimisation step per call on the HIP kernels: step(burst, frame_gt) -> loss (device scalar).

    net: a dbsr_amd DBSRNet on a HIP device (compute dtype bf16, fp32, or fp16 with the loss scaler: `loss_scale`,
    None / 'dynamic' / a fixed scale, with torch.amp.GradScaler's init_scale, growth_factor, backoff_factor and
    growth_interval; its state lives on the device, loss_scale_state() reads it).  Its DBSR parameters are
    re-pointed into one flat fp32 buffer (the optimizer's master copy; the module sees the updates);
    `flat_grad` holds the step's gradients in the same layout (decoder first, then merging, then
    encoder: the order the backward completes them, so the bucketed all-reduce can start early).

    flow_grad=True: the backward goes on to dL/d(offsets) -- the offset-feature extractor's first conv back to its
    2-channel input plus the warp's flow gradient (csrc/flow_grad.hip) -- and flow_grad() returns it, fp32
    [B,N-1,2,H,W] (unscaled when a loss scaler runs).  step / forward_backward / forward_saved take `flow`
    ([B,N-1,2,H,W] fp32 on the device): the offsets then come from the caller (an alignment network of their own)
    instead of the package's PWC-Net, in a plan of its own without PWC-Net ops.

    alignment_grad=True (a net built with train_alignmentnet=True; encoders.py:56-57): step(burst, frame_gt) also
    trains PWC-Net -- its differentiable forward (pwcnet.PWCNet, fp32) gives the flow, the external-flow plan runs
    with flow_grad, autograd carries flow_grad() into the PWC parameters (csrc/pwc_grad.hip) and dbsr_adam_step
    runs on a second flat buffer of them with the same lr, betas and eps; pwc_grad_view(p) is a PWC parameter's
    last gradient.  Not with loss_scale (so not fp16) and not with a world size above 1.  Without it such a net is
    refused.

    objective: None keeps the built-in L1 plan, op for op.  A metric name ('l1', 'l2', 'l2_sqrt', 'charbonnier') or
    an objectives.Objective makes the step's loss weight * metric + ssim * (1 - SSIM) + extra(pred, gt):
    dbsr_objective_step takes the place of the l1_loss_bwd op, an SSIM term adds dbsr_ssim_forward / _backward ops
    whose gradient it adds before the ReLU gate, and an `extra` callable (LPIPS with differentiable=True, any torch
    objective) runs eagerly between the plan's forward and backward on a leaf over the plan's prediction, its
    autograd gradient entering the same way.  Loss scaling, the bucketed all-reduce, graph replay and `flow=` work
    as without; step returns the total loss and `last_stats` holds Loss/total, Loss/rgb, Loss/raw/rgb, Stat/psnr
    and the extra terms as device tensors (the step reads nothing back).  A name takes the trainer's
    boundary_ignore, an Objective its own.  Not with optimizer=False; `extra` not with alignment_grad=True.
    """
    # re-pack every conv's weights in one launch (dbsr_conv_pack_weights_batch, bitwise the per-conv
    # pack / dgrad-transpose / pack launches it replaces: False runs those, for A/B and the equality test)
    BATCH_REPACK = True
    # forward: the weight predictor's output conv fused with the softmax + fusion (as the inference engine's
    # DBSREngine.FUSED_WP_OUT); False: the conv into a logits buffer + dbsr_fuse_softmax
    FUSED_WP_OUT = True

    def __init__(self, net, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, boundary_ignore=40, process_group=None,
                 bucket_bytes=4 << 20, optimizer=True, loss_scale=None, init_scale=65536.0, growth_factor=2.0,
                 backoff_factor=0.5, growth_interval=2000, flow_grad=False, alignment_grad=False, objective=None):
        dev = next(net.parameters()).device
        if dev.type != 'cuda':
            raise RuntimeError('DBSRTrainer needs the network on a HIP device')
        self.net, self.dev, self.dtype = net, dev, net.compute_dtype
        self.alignment_grad = bool(alignment_grad)
        self.objective = None
        if objective is not None:
            from .objectives import Objective
            if not optimizer:
                raise ValueError('DBSRTrainer: objective= belongs to the fused step; with optimizer=False (the '
                                 'autograd path) the caller computes the loss from the prediction')
            self.objective = Objective.of(objective, boundary_ignore)
            if self.objective.extra is not None and self.alignment_grad:
                raise NotImplementedError('DBSRTrainer: an objective with an `extra` callable is not supported with '
                                          'alignment_grad=True (both run eagerly around the plan)')
            boundary_ignore = self.objective.boundary_ignore
        self.want_flow_grad = bool(flow_grad) or self.alignment_grad
        self._flow_plan = None            # the plan whose dflow buffer holds the last backward's dL/d(offsets)
        # Loss scaling (csrc/loss_scale.hip, torch.amp.GradScaler's rule on the device).  None: no scaling -- the
        # plan and the optimizer launch are the unscaled ones -- except for an fp16 net, where it means 'dynamic':
        # the L1 gradient 1/count (~4.7e-8 at configs[3]) is below fp16's smallest subnormal, so an unscaled
        # fp16 backward underflows to zero.  A float is a fixed scale (no growth / backoff; steps
        # that overflow are still skipped).  The autograd path (optimizer=False) never scales: the caller's
        # GradScaler multiplies the loss, and the upstream gradient arrives scaled.
        if not optimizer:
            if loss_scale is not None:
                raise ValueError('DBSRTrainer: optimizer=False (the autograd path) does not scale internally; scale '
                                 'the loss with torch.amp.GradScaler')
        elif loss_scale is None and self.dtype == torch.float16:
            loss_scale = 'dynamic'
        self.scaling = loss_scale is not None
        if self.scaling:
            dynamic = isinstance(loss_scale, str)
            if dynamic and loss_scale != 'dynamic':
                raise ValueError("DBSRTrainer: loss_scale is None, 'dynamic' or a positive number, got %r" % (loss_scale,))
            scale0 = float(init_scale if dynamic else loss_scale)
            if not (scale0 > 0.0 and math.isfinite(scale0)):
                raise ValueError('DBSRTrainer: the loss scale must be positive and finite, got %r' % (scale0,))
            if not (growth_factor > 0.0 and backoff_factor > 0.0 and int(growth_interval) >= 1):
                raise ValueError('DBSRTrainer: growth_factor and backoff_factor must be > 0, growth_interval >= 1')
            # a fixed scale is the same update with both factors 1
            self.ls_args = (float(growth_factor), float(backoff_factor), int(growth_interval)) if dynamic \
                else (1.0, 1.0, int(growth_interval))
            # the scaler's state (dbsr_hip.h DBSR_LS_*): read and written by the kernels only during a step
            self._ls = torch.zeros(L.LS_WORDS, dtype=torch.int32, device=dev)
            self._ls.view(torch.float32)[L.LS_SCALE] = scale0
            self._fb_inf = torch.zeros(1, dtype=torch.int32, device=dev)   # found_inf of the last forward_backward
        self.lr, self.betas, self.eps, self.bi = lr, betas, eps, boundary_ignore
        if getattr(net.encoder, 'train_alignmentnet', False) and not self.alignment_grad:
            # the reference then backpropagates into PWC-Net (encoders.py:56-57); this trainer does so only when
            # asked (alignment_grad=True), so refuse rather than train without alignment gradients
            raise NotImplementedError('DBSRTrainer: train_alignmentnet=True (PWC-Net training) needs '
                                      'alignment_grad=True; or build the net with train_alignmentnet=False '
                                      '(dbsrnet_cvpr2021 default)')
        softmax, ref_base, self.offset_modulo = merging_variant(net.merging)
        if not (softmax and ref_base):
            # the backward kernels are the softmax's (dbsr_fuse_backward) and the reference-frame base's
            # (dbsr_merge_prep_backward); the inference engine runs these variants, training does not
            raise NotImplementedError('DBSRTrainer: WeightedSum(softmax=False / use_base_frame=False) is not on the '
                                      'HIP backward (dbsrnet_cvpr2021 defaults: softmax=True, use_base_frame=True)')
        self.pg = process_group
        self.world = dist.get_world_size(process_group) if (dist.is_available() and dist.is_initialized()) else 1
        if self.alignment_grad:
            # later work, both: the PWC backward runs unscaled through autograd, and its gradients are not bucketed
            if self.scaling:
                raise NotImplementedError('DBSRTrainer: loss_scale with alignment_grad=True is not supported (the '
                                          'PWC-Net backward is fp32 and unscaled)')
            if self.world > 1:
                raise NotImplementedError('DBSRTrainer: world size > 1 with alignment_grad=True is not supported (the '
                                          'PWC-Net gradients are not all-reduced)')
            self._init_alignment(optimizer)
        # PWC-Net runs without gradients (train_alignmentnet=False: encoders.py:58-61); its parameters are left
        # as the caller set them -- they never receive a .grad from this backward
        mods = self._trainable_convs()
        self.params = []
        for m in mods:
            self.params.append(m.weight)
            if m.bias is not None:
                self.params.append(m.bias)
        n = sum(p.numel() for p in self.params)
        self.flat = torch.empty(n, dtype=torch.float32, device=dev)
        self.flat_grad = torch.zeros(n, dtype=torch.float32, device=dev)
        # Adam moments (not allocated when an external optimizer steps the parameters: the autograd path)
        self.exp_avg = torch.zeros(n if optimizer else 0, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(n if optimizer else 0, dtype=torch.float32, device=dev)
        self.offset = {}
        o = 0
        for p in self.params:
            k = p.numel()
            self.flat[o:o + k].copy_(p.detach().reshape(-1).float())
            p.data = self.flat[o:o + k].view(p.shape)
            self.offset[id(p)] = (o, k)
            o += k
        self.n_params = n
        self.bucket_bytes = bucket_bytes
        self.step_count = 0
        self.plans = {}
        self.loss = torch.zeros(1, dtype=torch.float32, device=dev)
        if self.objective is not None:
            # dbsr_objective_step's {metric, weight * metric, weight / count}; the total is the weighted metric
            # itself unless SSIM / extra terms are added to it after the plan (device arithmetic, nothing read back)
            self._obj_loss = torch.zeros(3, dtype=torch.float32, device=dev)
            if self.objective.ssim is None and self.objective.extra is None:
                self.loss = self._obj_loss[1:2]
            self._obj_plan = None
        self.use_graph = True         # step(): replay the plan as HIP graphs after its first (eager) run
        self._pack()

    def _trainable_convs(self):
        return trainable_convs(self.net)

    def _init_alignment(self, optimizer):
        """The PWC-Net parameters as a second flat fp32 buffer with its own Adam moments: the reference gives
        net.parameters() to one Adam (default_synthetic.py:94), so lr, betas, eps and the step count are shared."""
        pwc = self.net.encoder.alignment_net
        if not getattr(pwc, 'differentiable', False):
            raise NotImplementedError('DBSRTrainer: alignment_grad=True needs the package\'s PWCNet with '
                                      'differentiable=True (dbsrnet_cvpr2021(train_alignmentnet=True))')
        self.pwc_params = [p for p in pwc.parameters() if p.requires_grad]
        if not optimizer:
            return
        n = sum(p.numel() for p in self.pwc_params)
        self.pwc_flat = torch.empty(n, dtype=torch.float32, device=self.dev)
        self.pwc_flat_grad = torch.zeros(n, dtype=torch.float32, device=self.dev)
        self.pwc_exp_avg = torch.zeros(n, dtype=torch.float32, device=self.dev)
        self.pwc_exp_avg_sq = torch.zeros(n, dtype=torch.float32, device=self.dev)
        self.pwc_offset = {}
        o = 0
        for p in self.pwc_params:
            k = p.numel()
            self.pwc_flat[o:o + k].copy_(p.detach().reshape(-1).float())
            p.data = self.pwc_flat[o:o + k].view(p.shape)
            self.pwc_offset[id(p)] = (o, k)
            o += k
        self.n_pwc_params = n

    def pwc_grad_view(self, p):
        """The last step's gradient of PWC-Net parameter p (a view of the flat gradient buffer)."""
        o, k = self.pwc_offset[id(p)]
        return self.pwc_flat_grad[o:o + k].view(p.shape)

    def _step_alignment(self, burst, frame_gt):
        """A step that also trains PWC-Net: its differentiable forward gives the flow, the external-flow plan runs
        with dL/d(offsets), autograd carries that into the PWC parameters, and both flat buffers take one Adam
        step."""
        from .dbsrnet import alignment_flow
        pwc = self.net.encoder.alignment_net
        with torch.enable_grad():
            flow = alignment_flow(self.net, burst.to(torch.float32))
        loss = self._step_plan(burst, frame_gt, flow.detach())
        grads = torch.autograd.grad(flow, self.pwc_params, self.flow_grad().to(flow.dtype), allow_unused=True)
        self.pwc_flat_grad.zero_()
        for p, g in zip(self.pwc_params, grads):
            if g is not None:
                self.pwc_grad_view(p).copy_(g)
        lib = L.lib()
        L.check(lib.dbsr_adam_step(self.n_pwc_params, self.pwc_flat.data_ptr(), self.pwc_flat_grad.data_ptr(),
                                   self.pwc_exp_avg.data_ptr(), self.pwc_exp_avg_sq.data_ptr(), self.lr, self.betas[0],
                                   self.betas[1], self.eps, self.step_count, 1.0, L.stream_ptr(self.dev)), 'adam (PWC)')
        # the parameters changed through their storage: packed copies keyed by tensor version are stale
        torch.ops.dbsr.clear_pack_cache()
        pwc._engine = None
        return loss

    def grad_view(self, p):
        o, k = self.offset[id(p)]
        return self.flat_grad.data_ptr() + 4 * o

    def _pack(self):
        net, dt, dev = self.net, self.dtype, self.dev
        enc, mer, dec = net.encoder, net.merging, net.decoder
        T = lambda m, shuffle=1: TConv(m, self, dt, dev, shuffle)                     # noqa: E731
        self.pwc = PWCPlanner(enc.alignment_net, _Weights(dt, dev, L.stream_ptr(dev)))
        self.enc_init = T(enc.init_layer[0])
        self.enc_res = [(T(b.conv1[0]), T(b.conv2[0])) for b in enc.res_layers]
        self.enc_out = T(enc.out_layer[0])
        self.proj = T(mer.feat_project_layer[0])
        ofe = list(mer.offset_feat_extractor)
        self.ofe_init = T(ofe[0][0])
        self.ofe_res = [(T(b.conv1[0]), T(b.conv2[0])) for b in ofe[1:]]
        wp = list(mer.weight_predictor)
        self.wp_init = T(wp[0][0])
        self.wp_res = [(T(b.conv1[0]), T(b.conv2[0])) for b in wp[1:-1]]
        self.wp_out = T(wp[-1][0])
        self.dec_init = T(dec.init_layer[0])
        self.dec_pre = [(T(b.conv1[0]), T(b.conv2[0])) for b in dec.pre_res_layers]
        up = dec.upsample_layer
        self.s = up.upsample_factor
        self.dec_up = T(up.conv_layer[0], shuffle=self.s)
        self.blur = gauss_kernel3(up.gauss_blur_sd, up.gauss_ksz) if up.gauss_blur_sd is not None else None
        self.dec_post = [(T(b.conv1[0]), T(b.conv2[0])) for b in dec.post_res_layers]
        self.pred = T(dec.predictor[0])
        if self.pred.cin != 32:
            # the predictor's forward / backward (dbsr_head_forward / dbsr_head_backward) take 32 input channels,
            # the reference's default dec_post_conv_dim: refuse here, not at the first step
            raise NotImplementedError('DBSRTrainer: dec_post_conv_dim = %d; the HIP predictor head trains 32 '
                                      'channels (dbsrnet_cvpr2021 default)' % self.pred.cin)
        # dgrad of the weight predictor's first conv, split: [base | diff] (ungated, to merge-prep) and the
        # offset features (gated by the offset-feature extractor's ReLU output)
        pd = self.proj.cout
        self.wp_init_bd = self.wp_init.sub_dgrad(0, 2 * pd, dt, dev)
        self.wp_init_of = self.wp_init.sub_dgrad(2 * pd, self.wp_init.cin, dt, dev)
        self.tconvs = [self.enc_init, self.enc_out, self.proj, self.ofe_init, self.wp_init, self.wp_out, self.dec_init,
                       self.dec_up, self.pred]
        for lst in (self.enc_res, self.ofe_res, self.wp_res, self.dec_pre, self.dec_post):
            for c1, c2 in lst:
                self.tconvs += [c1, c2]
        names = {id(m): n for n, m in net.named_modules()}
        for tc in self.tconvs:
            tc.name = names[id(tc.mod)]

    # ------------------------------------------------------------------------------------------------
    def _build(self, B, N, H, W, ext_flow=False, flow_grad=None):
        dt, dev, lib = self.dtype, self.dev, L.lib()
        flow_grad = self.want_flow_grad if flow_grad is None else bool(flow_grad)
        plan = Plan()
        plan.lane = 0
        F, P = B * N, B * (N - 1)
        C = self.enc_out.cout
        hw = (H, W)
        S = self.s
        bufs = {'burst': torch.zeros(B, N, 4, H, W, dtype=torch.float32, device=dev)}
        ws_req = []

        def ws(kind, nbytes):
            w = _WS(kind, nbytes)
            ws_req.append(w)
            return w

        def wgrad(name, tc, n, h, w, x, xc0, dy, dyc0, xmap=IDENTITY, dymap=IDENTITY, accumulate=0, cin=None, cout=None):
            """weight gradient, and the bias gradient (when the conv has one) from the same pass over dy"""
            ci = tc.cin if cin is None else cin
            co = tc.cout if cout is None else cout
            need = lib.dbsr_conv_wgrad_workspace_bytes(n, h, w, ci, co, tc.k)
            work = ('flop', 2.0 * n * h * w * ci * co * tc.k * tc.k)
            if tc.gb is None:
                plan.add('wgrad.' + name, lib.dbsr_conv_wgrad, n, h, w, x.d(xc0, xmap), ci, dy.d(dyc0, dymap), co,
                         tc.k, tc.gw, accumulate, ws('wg', need), need, work=work)
            else:
                plan.add('wgrad.' + name, lib.dbsr_conv_wgrad_bias, n, h, w, x.d(xc0, xmap), ci, dy.d(dyc0, dymap),
                         co, tc.k, tc.gw, tc.gb, accumulate, ws('wg', need), need, work=work)
            plan.kernel[len(plan.ops) - 1] = 'conv_wgrad'

        # ================= forward with saved activations =================
        if DBSRTrainer.BATCH_REPACK:
            # every conv's forward and dgrad weights re-packed from the updated fp32 master in one launch
            jobs = [j for tc in self.tconvs for j in tc.pack_jobs()]
            arr = (L.PackJob * len(jobs))(*jobs)
            nblk = lib.dbsr_pack_batch_prepare(arr, len(jobs))
            if nblk < 0:
                L.check(-1, 'dbsr_pack_batch_prepare')
            table = torch.frombuffer(bytearray(arr), dtype=torch.uint8).to(dev)
            plan.keep.append(table)
            plan.add('repack.all', lib.dbsr_conv_pack_weights_batch, table.data_ptr(), len(jobs), nblk)
        else:
            for tc in self.tconvs:
                tc.repack_ops(plan)
        raw = NHWC(F, H, W, 8, dt, dev)
        Hp, Wp = int(math.ceil(H / 64.0) * 64), int(math.ceil(W / 64.0) * 64)
        offsets = torch.zeros(P, 2, H, W, dtype=torch.float32, device=dev)
        om = NHWC(F, H, W, 8, dt, dev)
        if ext_flow:
            # the caller's offsets: no PWC-Net ops (and no RGB frames for it); `offsets` is a copy, `om` as
            # dbsr_flow_finalize writes it
            if P == 0:
                raise ValueError('DBSRTrainer: external flows need a burst of at least two frames')
            rgb = flow_out = None
            bufs['flow'] = torch.zeros(P, 2, H, W, dtype=torch.float32, device=dev)
            plan.add('pack_burst', lib.dbsr_pack_burst, B, N, H, W, bufs['burst'].data_ptr(), raw.d(0), Hp, Wp,
                     L.NULL_TENSOR)
            plan.add('offsets_export', lib.dbsr_offsets_export, B, N, H, W, bufs['flow'].data_ptr(), 2 * H * W,
                     offsets.data_ptr(), self.offset_modulo, om.d(0))
        else:
            rgb = NHWC(F, Hp, Wp, 8, dt, dev)
            plan.add('pack_burst', lib.dbsr_pack_burst, B, N, H, W, bufs['burst'].data_ptr(), raw.d(0), Hp, Wp,
                     rgb.d(0))
            flow_out = NHWC(P, Hp // 4, Wp // 4, 2, torch.float32, dev)
            self.pwc.build(plan, dt, dev, F, Hp, Wp, P, first_map=(N - 1, N, 0, 0), second_map=(N - 1, N, 1, 1),
                           rgb=rgb, flow_out=flow_out)
            plan.add('flow_finalize', lib.dbsr_flow_finalize, B, N, Hp // 4, Wp // 4, flow_out.d(0), H, W, Hp, Wp,
                     offsets.data_ptr(), self.offset_modulo, om.d(0))

        def res_fwd(name, blocks, n, hw_, x, xc0, width, last_out=None):
            """ResBlocks with every activation kept: returns [(x, xc0, t, y, yc0)] per block."""
            saved = []
            for i, (c1, c2) in enumerate(blocks):
                t = NHWC(n, hw_[0], hw_[1], r8(width), dt, dev)
                if i == len(blocks) - 1 and last_out is not None:
                    y, yc0 = last_out
                else:
                    y, yc0 = NHWC(n, hw_[0], hw_[1], r8(width), dt, dev), 0
                plan.conv(f'{name}{i}.conv1', c1.fwd, n, x, xc0, hw_, t, 0, L.ACT_RELU)
                plan.conv(f'{name}{i}.conv2', c2.fwd, n, t, 0, hw_, y, yc0, L.ACT_NONE, res=x, rc0=xc0,
                          post_act=L.ACT_RELU)
                saved.append((x, xc0, t, y, yc0))
                x, xc0 = y, yc0
            return saved

        pd, od = self.proj.cout, self.ofe_init.cout
        WP = NHWC(F, H, W, 2 * pd + od, dt, dev)
        o0 = NHWC(F, H, W, od, dt, dev)
        plan.conv('ofe.init', self.ofe_init.fwd, F, om, 0, hw, o0, 0, L.ACT_RELU)
        ofe_s = res_fwd('ofe.res', self.ofe_res, F, hw, o0, 0, od, last_out=(WP, 2 * pd))
        e0 = NHWC(F, H, W, r8(self.enc_init.cout), dt, dev)
        plan.conv('enc.init', self.enc_init.fwd, F, raw, 0, hw, e0, 0, L.ACT_RELU)
        enc_s = res_fwd('enc.res', self.enc_res, F, hw, e0, 0, self.enc_init.cout)
        e_last = enc_s[-1][3] if enc_s else e0
        E = NHWC(F, H, W, C, dt, dev)
        plan.conv('enc.out', self.enc_out.fwd, F, e_last, 0, hw, E, 0, L.ACT_RELU)
        PJ = NHWC(F, H, W, r8(pd), dt, dev)
        plan.conv('proj_ref', self.proj.fwd, B, E, 0, hw, PJ, 0, L.ACT_RELU, xmap=(1, N, 0, 1), ymap=(1, N, 0, 1))
        Wf = NHWC(max(P, 1), H, W, C, dt, dev)
        plan.add('warp', lib.dbsr_warp_bilinear, P, H, W, C, E.d(0, (N - 1, N, 1, 1)), offsets.data_ptr(), 2 * H * W,
                 Wf.d(0))
        plan.conv('proj_oth', self.proj.fwd, P, Wf, 0, hw, PJ, 0, L.ACT_RELU, ymap=(N - 1, N, 1, 1))
        plan.add('merge_prep', lib.dbsr_merge_prep, B, N, H * W, pd, PJ.d(0), WP.d(0))
        qw = self.wp_init.cout
        q0 = NHWC(F, H, W, qw, dt, dev)
        plan.conv('wp.init', self.wp_init.fwd, F, WP, 0, hw, q0, 0, L.ACT_RELU)
        wp_s = res_fwd('wp.res', self.wp_res, F, hw, q0, 0, qw)
        q_last = wp_s[-1][3] if wp_s else q0
        FUS = NHWC(B, H, W, C, dt, dev)
        FW = NHWC(F, H, W, C, dt, dev)
        # the weight predictor's output conv + softmax + fusion in one launch (dbsr_conv_fuse_softmax, fp32 logits
        # that never reach memory: the backward needs only the weights FW, merging.py:116-124) where the library
        # serves the shape; else the conv into 16-bit logits + dbsr_fuse_softmax
        LG = None
        if not (DBSRTrainer.FUSED_WP_OUT and plan.conv_fuse('wp.out+fuse', self.wp_out.fwd, B, N, q_last, hw,
                                                             E.d(0, (1, N, 0, 1)), Wf.d(0), FUS.d(0), FW.d(0))
                is not None):
            LG = NHWC(F, H, W, C, dt, dev)
            plan.conv('wp.out', self.wp_out.fwd, F, q_last, 0, hw, LG, 0, L.ACT_NONE)
            plan.add('fuse', lib.dbsr_fuse_softmax, B, N, H * W, C, LG.d(0), E.d(0, (1, N, 0, 1)), Wf.d(0), FUS.d(0),
                     FW.d(0))
        gd = self.dec_init.cout
        g0 = NHWC(B, H, W, gd, dt, dev)
        plan.conv('dec.init', self.dec_init.fwd, B, FUS, 0, hw, g0, 0, L.ACT_RELU)
        pre_s = res_fwd('dec.pre', self.dec_pre, B, hw, g0, 0, gd)
        g_last = pre_s[-1][3] if pre_s else g0
        pc = self.dec_up.cout // (S * S)
        HS, WS = H * S, W * S
        S0 = NHWC(B, HS, WS, pc, dt, dev)
        plan.conv('dec.upsample', self.dec_up.fwd, B, g_last, 0, hw, S0, 0, L.ACT_RELU, out_mode=L.OUT_SHUFFLE,
                  shuffle=S)
        if self.blur is not None:
            S1 = NHWC(B, HS, WS, pc, dt, dev)
            kbuf = (ctypes.c_float * 9)(*self.blur)
            kflip = (ctypes.c_float * 9)(*self.blur[::-1])       # correlation^T = correlation with the flipped kernel
            plan.keep.extend([kbuf, kflip])
            plan.add('dec.blur', lib.dbsr_gauss_blur3, B, HS, WS, pc, S0.d(0), kbuf, S1.d(0))
        else:
            S1 = S0
        post_s = res_fwd('dec.post', self.dec_post, B, (HS, WS), S1, 0, pc)
        h_last = post_s[-1][3] if post_s else S1
        hc = self.pred.cout
        pred = torch.zeros(B, hc, HS, WS, dtype=torch.float32, device=dev)
        # the predictor on its own (h_last is kept for the backward): fp32 weights, fp32 NCHW out
        pmod = self.pred.mod
        plan.add('dec.predictor', lib.dbsr_head_forward, B, HS * WS, h_last.d(0), pc, pmod.weight.data_ptr(),
                 pmod.bias.data_ptr() if pmod.bias is not None else None, hc, pred.data_ptr(),
                 work=('flop', 2.0 * B * HS * WS * pc * hc))
        bufs['pred'] = pred
        bufs['offsets'] = offsets
        bufs['gt'] = torch.zeros(B, 3, HS, WS, dtype=torch.float32, device=dev)

        # ================= backward =================
        plan.add('zero_grad', lib.dbsr_zero, self.flat_grad.data_ptr(), self.flat_grad.numel() * 4)
        buckets = []                     # (op index after which this bucket's grads are final, lo, hi)

        def mark_bucket(tc_list):
            lo = min(self.offset[id(p)][0] for tc in tc_list for p in ([tc.mod.weight] + ([tc.mod.bias] if tc.mod.bias is not None else [])))
            hi = max(sum(self.offset[id(p)]) for tc in tc_list for p in ([tc.mod.weight] + ([tc.mod.bias] if tc.mod.bias is not None else [])))
            buckets.append((len(plan.ops), lo, hi))

        dP = NHWC(B, HS, WS, 8, dt, dev)
        nlb = (B * HS * WS + 255) // 256
        plan.fwd_end = len(plan.ops)            # ops[:fwd_end]: the forward with saved activations (+ grad zeroing)
        obj = self.objective
        if obj is not None:
            # the objective's ops: [ssim_fwd, ssim_bwd,] <metric>_loss_bwd.  The SSIM gradient of ssim * (1 - SSIM)
            # lands in `gextra` (its scale -ssim / (3 B Hm Wm + 1e-12) is a constant without a mask: a device scalar
            # written once); an `extra` callable's gradient is added there eagerly, before plan.obj_op runs
            gextra = None
            if obj.ssim is not None or obj.extra is not None:
                gextra = bufs['gextra'] = torch.zeros(B, 3, HS, WS, dtype=torch.float32, device=dev)
            if obj.ssim is not None:
                need = lib.dbsr_ssim_workspace_bytes(B, 3, HS, WS, self.bi)
                if need == 0:
                    raise ValueError('DBSRTrainer: the SSIM term needs a crop of at least 11 x 11 pixels, got %d x %d'
                                     % (HS - 2 * self.bi, WS - 2 * self.bi))
                sws = torch.zeros(need, dtype=torch.uint8, device=dev)
                plan.ssim_result = torch.zeros(2, dtype=torch.float32, device=dev)
                ssums = torch.zeros(B, 2, dtype=torch.float32, device=dev)
                windows = 3.0 * B * (HS - 2 * self.bi - 10) * (WS - 2 * self.bi - 10)
                sscale = torch.full((1,), -obj.ssim / (windows + 1e-12), dtype=torch.float32, device=dev)
                plan.keep.extend([sws, ssums, sscale])
                plan.add('ssim_fwd', lib.dbsr_ssim_forward, B, 3, HS, WS, self.bi, pred.data_ptr(),
                         bufs['gt'].data_ptr(), None, obj.ssim_val_range, None, ssums.data_ptr(),
                         plan.ssim_result.data_ptr(), sws.data_ptr(), need)
                plan.add('ssim_bwd', lib.dbsr_ssim_backward, B, 3, HS, WS, self.bi, pred.data_ptr(),
                         bufs['gt'].data_ptr(), None, obj.ssim_val_range, sscale.data_ptr(), gextra.data_ptr(), None, 0)
            plan.obj_op = len(plan.ops)
            plan.obj_stats = torch.zeros(B, 2, dtype=torch.float64, device=dev)
            need = lib.dbsr_objective_workspace_bytes(B, HS, WS)
            plan.add(obj.metric + '_loss_bwd', lib.dbsr_objective_step, B, HS, WS, self.bi, L.METRIC_CODES[obj.metric],
                     obj.weight, pred.data_ptr(), bufs['gt'].data_ptr(),
                     gextra.data_ptr() if gextra is not None else None,
                     self._ls.data_ptr() if self.scaling else None, dP.d(0), self._obj_loss.data_ptr(),
                     plan.obj_stats.data_ptr(), ws('obj', need), need)
        elif self.scaling:
            # dP = scale * dL/dpre with the scale read from the scaler's state on the device (the loss stays unscaled)
            plan.add('l1_loss_bwd', lib.dbsr_l1_loss_backward_scaled, B, 3, HS, WS, self.bi, pred.data_ptr(),
                     bufs['gt'].data_ptr(), self._ls.data_ptr(), dP.d(0), self.loss.data_ptr(), ws('l1', 4 * nlb),
                     4 * nlb)
        else:
            plan.add('l1_loss_bwd', lib.dbsr_l1_loss_backward, B, 3, HS, WS, self.bi, pred.data_ptr(),
                     bufs['gt'].data_ptr(), dP.d(0), self.loss.data_ptr(), ws('l1', 4 * nlb), 4 * nlb)
        # autograd: the same backward from an upstream dL/dpred instead of the built-in L1 objective
        bufs['gpred'] = torch.zeros(B, 3, HS, WS, dtype=torch.float32, device=dev)
        plan.grad_in_op = (lib.dbsr_relu_grad, (B, 3, HS, WS, pred.data_ptr(), bufs['gpred'].data_ptr(), dP.d(0)),
                           'relu_grad', 0)
        # predictor backward in one pass over dP and h_last: its dgrad gated by h_last's ReLU, weight and bias grads
        gh = NHWC(B, HS, WS, r8(pc), dt, dev)
        need = lib.dbsr_head_backward_workspace_bytes(B, HS * WS, pc, hc)
        plan.add('bwd.dec.predictor', lib.dbsr_head_backward, B, HS * WS, h_last.d(0), pc, dP.d(0),
                 pmod.weight.data_ptr(), hc, gh.d(0), self.pred.gw, self.pred.gb, 0, ws('hb', need), need,
                 work=('flop', 4.0 * B * HS * WS * pc * hc))

        def res_bwd(name, blocks, saved, n, hw_, g, gc0, gate_first):
            """ResBlock backward (blocks.py:81-96) from g = dL/dy * [y > 0]; returns the gradient w.r.t. the
            chain's input, gated by that input's ReLU when gate_first (else ungated)."""
            for i in reversed(range(len(blocks))):
                c1, c2 = blocks[i]
                x, xc0, t, y, yc0 = saved[i]
                dt_ = NHWC(n, hw_[0], hw_[1], t.ld, dt, dev)
                plan.conv(f'bwd.{name}{i}.conv2', c2.bwd, n, g, gc0, hw_, dt_, 0, L.ACT_NONE, gate=t)
                wgrad(f'{name}{i}.conv2', c2, n, hw_[0], hw_[1], t, 0, g, gc0)
                dx = NHWC(n, hw_[0], hw_[1], t.ld, dt, dev)
                gate = x if (i > 0 or gate_first) else None
                plan.conv(f'bwd.{name}{i}.conv1', c1.bwd, n, dt_, 0, hw_, dx, 0, L.ACT_NONE, res=g, rc0=gc0,
                          gate=gate, gc0=xc0 if gate is not None else 0)
                wgrad(f'{name}{i}.conv1', c1, n, hw_[0], hw_[1], x, xc0, dt_, 0)
                plan.keep.extend([dt_, dx])         # launches hold raw pointers: the plan owns every buffer
                g, gc0 = dx, 0
            return g, gc0

        dS1, _ = res_bwd('dec.post', self.dec_post, post_s, B, (HS, WS), gh, 0, gate_first=False)
        if self.blur is not None:
            dS0 = NHWC(B, HS, WS, pc, dt, dev)
            plan.add('bwd.dec.blur', lib.dbsr_gauss_blur3, B, HS, WS, pc, dS1.d(0), kflip, dS0.d(0))
        else:
            dS0 = dS1
        dU = NHWC(B, H, W, self.dec_up.cout, dt, dev)
        plan.add('bwd.dec.unshuffle', lib.dbsr_unshuffle_gate, B, H, W, S, pc, dS0.d(0), S0.d(0), dU.d(0))
        wgrad('dec.upsample', self.dec_up, B, H, W, g_last, 0, dU, 0)
        gp = NHWC(B, H, W, gd, dt, dev)
        plan.conv('bwd.dec.upsample', self.dec_up.bwd, B, dU, 0, hw, gp, 0, L.ACT_NONE, gate=g_last)
        gi, _ = res_bwd('dec.pre', self.dec_pre, pre_s, B, hw, gp, 0, gate_first=True)
        if not pre_s:
            pass
        wgrad('dec.init', self.dec_init, B, H, W, FUS, 0, gi, 0)
        dFUS = NHWC(B, H, W, C, dt, dev)
        plan.conv('bwd.dec.init', self.dec_init.bwd, B, gi, 0, hw, dFUS, 0, L.ACT_NONE)
        mark_bucket([self.pred, self.dec_up, self.dec_init] + [c for blk in self.dec_pre + self.dec_post for c in blk])
        # fusion
        dLG = NHWC(F, H, W, C, dt, dev)
        dF0 = NHWC(B, H, W, C, dt, dev)
        dWfF = NHWC(max(P, 1), H, W, C, dt, dev)
        plan.add('bwd.fuse', lib.dbsr_fuse_backward, B, N, H * W, C, FW.d(0), E.d(0, (1, N, 0, 1)), Wf.d(0), FUS.d(0),
                 dFUS.d(0), dLG.d(0), dF0.d(0), dWfF.d(0))
        # weight predictor
        wgrad('wp.out', self.wp_out, F, H, W, q_last, 0, dLG, 0)
        gq = NHWC(F, H, W, qw, dt, dev)
        plan.conv('bwd.wp.out', self.wp_out.bwd, F, dLG, 0, hw, gq, 0, L.ACT_NONE, gate=q_last)
        gq0, _ = res_bwd('wp.res', self.wp_res, wp_s, F, hw, gq, 0, gate_first=True)
        wgrad('wp.init', self.wp_init, F, H, W, WP, 0, gq0, 0)
        dWP = NHWC(F, H, W, 2 * pd + od, dt, dev)
        plan.conv('bwd.wp.init.bd', self.wp_init_bd, F, gq0, 0, hw, dWP, 0, L.ACT_NONE)
        plan.conv('bwd.wp.init.of', self.wp_init_of, F, gq0, 0, hw, dWP, 2 * pd, L.ACT_NONE, gate=WP, gc0=2 * pd)
        # offset-feature extractor (the gradient that reaches its input, offsets % modulo, is taken below with
        # flow_grad; without it the offsets are a constant)
        go, go_c0 = res_bwd('ofe.res', self.ofe_res, ofe_s, F, hw, dWP, 2 * pd, gate_first=True)
        wgrad('ofe.init', self.ofe_init, F, H, W, om, 0, go, 0)
        # merge prep + projection
        dPJ = NHWC(F, H, W, r8(pd), dt, dev)
        plan.add('bwd.merge_prep', lib.dbsr_merge_prep_backward, B, N, H * W, pd, dWP.d(0), PJ.d(0), dPJ.d(0))
        wgrad('proj.ref', self.proj, B, H, W, E, 0, dPJ, 0, xmap=(1, N, 0, 1), dymap=(1, N, 0, 1))
        if P > 0:
            wgrad('proj.oth', self.proj, P, H, W, Wf, 0, dPJ, 0, dymap=(N - 1, N, 1, 1), accumulate=1)
        mark_bucket([self.wp_out, self.wp_init, self.ofe_init, self.proj] +
                    [c for blk in self.wp_res + self.ofe_res for c in blk])
        dEref = NHWC(B, H, W, C, dt, dev)
        plan.conv('bwd.proj.ref', self.proj.bwd, B, dPJ, 0, hw, dEref, 0, L.ACT_NONE, xmap=(1, N, 0, 1), res=dF0)
        dWf = NHWC(max(P, 1), H, W, C, dt, dev)
        dE = NHWC(F, H, W, C, dt, dev)
        if P > 0:
            plan.conv('bwd.proj.oth', self.proj.bwd, P, dPJ, 0, hw, dWf, 0, L.ACT_NONE, xmap=(N - 1, N, 1, 1), res=dWfF)
            # warp backward (owner-computes gather, no atomics) straight into the other frames' encoder-output
            # gradient, gated by the encoder's output ReLU (encoders.py:66-80)
            need = lib.dbsr_warp_backward_gather_workspace_bytes(P, H, W)
            plan.add('bwd.warp', lib.dbsr_warp_backward_gather, P, H, W, C, dWf.d(0), offsets.data_ptr(), 2 * H * W,
                     E.d(0, (N - 1, N, 1, 1)), dE.d(0, (N - 1, N, 1, 1)), ws('wb', need), need)
        plan.dflow = None
        if flow_grad and P > 0:
            # dL/d(offsets), fp32 [P][2][H][W]: the offset-feature extractor's first conv back to its 2-channel
            # input for the frames n >= 1 (go is gated; the modulo has derivative 1; the reference frame's offsets
            # are a constant) written by the dgrad conv's fp32 NCHW epilogue, then the warp's flow gradient added
            plan.dflow = torch.zeros(P, 2, H, W, dtype=torch.float32, device=dev)
            ddesc = L.tensor_desc(plan.dflow, 1, 0, img_stride=2 * H * W, dtype=torch.float32)
            plan.conv('bwd.ofe.init.dgrad', self.ofe_init.bwd, P, go, go_c0, hw, None, 0, L.ACT_NONE,
                      xmap=(N - 1, N, 1, 1), out_mode=L.OUT_NCHW_F32, y_desc=ddesc)
            plan.add('bwd.warp.flow', lib.dbsr_warp_flow_backward, P, H, W, C, E.d(0, (N - 1, N, 1, 1)), dWf.d(0),
                     offsets.data_ptr(), 2 * H * W, plan.dflow.data_ptr(), 2 * H * W, 1,
                     work=('byte', float(P) * H * W * C * dWf.t.element_size() * 5))
        plan.add('bwd.enc.gate', lib.dbsr_gate_copy, B, H * W, C, dEref.d(0), E.d(0, (1, N, 0, 1)),
                 dE.d(0, (1, N, 0, 1)))
        # encoder
        wgrad('enc.out', self.enc_out, F, H, W, e_last, 0, dE, 0)
        ge = NHWC(F, H, W, r8(self.enc_init.cout), dt, dev)
        plan.conv('bwd.enc.out', self.enc_out.bwd, F, dE, 0, hw, ge, 0, L.ACT_NONE, gate=e_last)
        ge0, _ = res_bwd('enc.res', self.enc_res, enc_s, F, hw, ge, 0, gate_first=True)
        wgrad('enc.init', self.enc_init, F, H, W, raw, 0, ge0, 0)
        mark_bucket([self.enc_init, self.enc_out] + [c for blk in self.enc_res for c in blk])
        # ---- scratch: one buffer per kind, as large as its largest request ----
        sizes = {}
        for w in ws_req:
            sizes[w.kind] = max(sizes.get(w.kind, 0), w.nbytes)
        scratch = {k: torch.zeros(max(v // 4, 1), dtype=torch.float32, device=dev) for k, v in sizes.items()}
        for i, (fn, args, name, lane) in enumerate(plan.ops):
            if any(isinstance(a, _WS) for a in args):
                plan.ops[i] = (fn, tuple(scratch[a.kind].data_ptr() if isinstance(a, _WS) else a for a in args), name,
                               lane)
        plan.finalize_workspace(dev)
        plan.keep.extend([raw, rgb, om, flow_out, WP, o0, e0, E, PJ, Wf, q0, LG, FUS, FW, g0, S0, S1, dP, gh, dS0, dU,
                          gp, dFUS, dLG, dF0, dWfF, gq, dWP, dPJ, dEref, dWf, dE, ge, ofe_s, enc_s, wp_s, pre_s,
                          post_s, scratch])
        plan.bufs = bufs
        plan.buckets = buckets
        plan.FW, plan.gen = FW, 0
        plan.dP = dP                    # the ReLU-gated NHWC dL/dpred the backward ops consume (objective hooks)
        plan.graphs, plan.eager_runs = None, 0      # HIP graphs of the step's segments (DBSRTrainer.step)
        return plan

    # ------------------------------------------------------------------------------------------------
    def step(self, burst, frame_gt, flow=None):
        """One training step on this rank's bursts [B,N,4,H,W] and ground truth [B,3,sH,sW] (flow: the caller's
        offsets [B,N-1,2,H,W] instead of PWC-Net's); returns the rank-local loss (device tensor, shape [1]).  With
        alignment_grad=True and no `flow`, PWC-Net is trained too."""
        if self.alignment_grad and flow is None:
            return self._step_alignment(burst, frame_gt)
        return self._step_plan(burst, frame_gt, flow)

    def _step_plan(self, burst, frame_gt, flow=None):
        plan = self._load(burst, frame_gt, flow)
        stream = L.stream_ptr(self.dev)
        # segments of the op list between the gradient buckets' completion points: each segment is one HIP
        # graph replay (after one eager step), and a bucket's all-reduce is issued right after its segment.  An
        # objective's `extra` callable runs eagerly before the objective's op: one more cut
        eager_at = plan.obj_op if (self.objective is not None and self.objective.extra is not None) else None
        cuts = [0] + ([eager_at] if eager_at is not None else []) + \
            ([b[0] for b in plan.buckets] if self.world > 1 else []) + [len(plan.ops)]
        segs = [(a, b) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]
        if self.use_graph and plan.graphs is None and plan.eager_runs > 0:
            plan.graphs = []
            for a, b in segs:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    plan.run_list(plan.ops[a:b], L.stream_ptr(self.dev))
                plan.graphs.append(g)
        works = []
        bi = 0
        for si, (a, b) in enumerate(segs):
            if plan.graphs is not None:
                plan.graphs[si].replay()
            else:
                plan.run_list(plan.ops[a:b], stream)
            if b == eager_at:
                self._objective_extra(plan)
            while bi < len(plan.buckets) and plan.buckets[bi][0] == b:
                if self.world > 1:
                    _, lo, hi = plan.buckets[bi]
                    works.append(allreduce_bucket(self.flat_grad, lo, hi, self.pg))
                bi += 1
        plan.eager_runs += 1
        for w_ in works:
            w_.wait()
        self._objective_total(plan)
        self._optimizer_step(stream)
        return self.loss.clone()          # (self.loss is the plan's buffer, overwritten by the next step)

    def _objective_extra(self, plan):
        """The objective's `extra` term on a leaf over the plan's prediction; its gradient goes into the plan's
        gextra buffer (added to the SSIM term's when there is one), which the objective's op reads next."""
        pred = plan.bufs['pred'].detach().requires_grad_(True)
        with torch.enable_grad():
            value = self.objective.extra(pred, plan.bufs['gt'])
            (g,) = torch.autograd.grad(value, pred)
        if self.objective.ssim is not None:
            plan.bufs['gextra'].add_(g.to(torch.float32))
        else:
            plan.bufs['gextra'].copy_(g.to(torch.float32))
        plan.extra_value = value.detach().to(torch.float32).reshape(1)

    def _objective_total(self, plan):
        """Loss/total of a step with an objective: the weighted metric plus the SSIM and extra terms, on the device."""
        obj = self.objective
        if obj is None:
            return
        self._obj_plan = plan
        if obj.ssim is None and obj.extra is None:
            return                                      # self.loss is the weighted metric's own buffer
        total = self._obj_loss[1:2].clone()
        if obj.ssim is not None:
            total += obj.ssim * (1.0 - plan.ssim_result[:1])
        if obj.extra is not None:
            total += plan.extra_value
        self.loss = total

    @property
    def last_stats(self):
        """The reference actor's statistics of the last step with an objective (actors/dbsr_actors.py:35-45) as
        device tensors of shape [1] -- Loss/total, Loss/rgb (weight * metric), Loss/raw/rgb, Stat/psnr, and
        Loss/ssim, Loss/raw/ssim, Loss/extra for the terms the objective has; None before the first step or without
        an objective.  Stat/psnr is one small launch here (dbsr_psnr_from_stats); nothing is read back."""
        obj, plan = self.objective, getattr(self, '_obj_plan', None)
        if obj is None or plan is None:
            return None
        st = {'Loss/total': self.loss.clone(), 'Loss/rgb': self._obj_loss[1:2].clone(),
              'Loss/raw/rgb': self._obj_loss[0:1].clone()}
        if obj.ssim is not None:
            raw = 1.0 - plan.ssim_result[:1]
            st['Loss/raw/ssim'], st['Loss/ssim'] = raw, obj.ssim * raw
        if obj.extra is not None:
            st['Loss/extra'] = plan.extra_value.clone()
        if obj.psnr:
            out = torch.zeros(1, dtype=torch.float32, device=self.dev)
            L.check(L.lib().dbsr_psnr_from_stats(plan.obj_stats.shape[0], plan.obj_stats.data_ptr(), 0, 1.0, None,
                                                 out.data_ptr(), None, L.stream_ptr(self.dev)), 'psnr_from_stats')
            st['Stat/psnr'] = out
        return st

    def _optimizer_step(self, stream):
        self.step_count += 1
        lib = L.lib()
        self._unscale_flow_grad(stream)
        if self.scaling:
            # Order (step() calls this after every bucket's all-reduce has completed, before anything else touches
            # the gradients): unscale + overflow check on the SUMMED gradients, then the guarded Adam, then the
            # scaler's update.  The all-reduce is a sum, so an inf / NaN on one rank is an inf / NaN in every
            # rank's flat_grad: all ranks set found_inf alike and take the same skip / backoff decision from
            # their own copy of the state, without a second collective; the states stay equal step after step.
            # Nothing here is read back: the decision, the scale and Adam's t stay on the device.
            L.check(lib.dbsr_grad_unscale_check(self.n_params, self.flat_grad.data_ptr(), self._ls.data_ptr(),
                                                stream), 'grad_unscale_check')
            L.check(lib.dbsr_adam_step_guarded(self.n_params, self.flat.data_ptr(), self.flat_grad.data_ptr(),
                                               self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), self.lr,
                                               self.betas[0], self.betas[1], self.eps, 1.0 / self.world,
                                               self._ls.data_ptr(), stream), 'adam_step_guarded')
            L.check(lib.dbsr_loss_scale_update(self._ls.data_ptr(), *self.ls_args, stream), 'loss_scale_update')
        else:
            L.check(lib.dbsr_adam_step(self.n_params, self.flat.data_ptr(), self.flat_grad.data_ptr(),
                                       self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), self.lr, self.betas[0],
                                       self.betas[1], self.eps, self.step_count, 1.0 / self.world, stream), 'adam')
        # the inference engine packs from the module parameters (now updated in place through their storage):
        # it re-packs them into its existing buffers at its next forward, keeping its plans and graphs
        eng = getattr(self.net, '_engine', None)
        if eng is not None:
            eng.weights_stale = True

    def forward_backward(self, burst, frame_gt, flow=None):
        """Loss and gradients only (no all-reduce, no optimizer step): for tests."""
        plan = self._load(burst, frame_gt, flow)
        if self.objective is not None and self.objective.extra is not None:
            plan.run_list(plan.ops[:plan.obj_op], L.stream_ptr(self.dev))
            self._objective_extra(plan)
            plan.run_list(plan.ops[plan.obj_op:], L.stream_ptr(self.dev))
        else:
            plan.run(L.stream_ptr(self.dev))
        self._objective_total(plan)
        self._unscale_only(L.stream_ptr(self.dev))
        return self.loss, plan.bufs['pred']

    def _load(self, burst, frame_gt, flow=None, flow_grad=None):
        """The plan of this burst shape (the PWC-Net plan, or with `flow` the external-flow plan) with its inputs
        copied in."""
        plan = self._plan(burst.shape, flow, flow_grad)
        plan.bufs['burst'].copy_(burst.to(torch.float32), non_blocking=True)
        if frame_gt is not None:
            plan.bufs['gt'].copy_(frame_gt.to(torch.float32), non_blocking=True)
        if flow is not None:
            plan.bufs['flow'].copy_(flow.detach().to(torch.float32).reshape(plan.bufs['flow'].shape),
                                    non_blocking=True)
        self._flow_plan = plan
        return plan

    def flow_grad(self):
        """dL/d(offsets) of the last backward, fp32 [B,N-1,2,H,W] (a view of the plan's buffer, overwritten by the
        next backward of the same plan; unscaled when a loss scaler runs).  Needs flow_grad=True."""
        plan = self._flow_plan
        if plan is None or plan.dflow is None:
            raise RuntimeError('DBSRTrainer.flow_grad(): build the trainer with flow_grad=True and run a backward '
                               '(a burst of at least two frames)')
        B, N = plan.bufs['burst'].shape[:2]
        return plan.dflow.view(B, N - 1, *plan.dflow.shape[1:])

    def _unscale_flow_grad(self, stream):
        """With a loss scaler the backward ran on the scaled loss: divide dL/d(offsets) by the scale on the device
        (dbsr_grad_unscale_check, which also raises found_inf on an overflow); nothing is read back.  Whatever
        non-finite value reaches this rank-local buffer also reaches a parameter gradient (dWf feeds bwd.warp, go
        feeds wgrad.ofe.init), which the all-reduce carries to every rank: the ranks still decide alike."""
        plan = self._flow_plan
        if self.scaling and plan is not None and plan.dflow is not None:
            L.check(L.lib().dbsr_grad_unscale_check(plan.dflow.numel(), plan.dflow.data_ptr(), self._ls.data_ptr(),
                                                    stream), 'grad_unscale_check')

    def _unscale_only(self, stream):
        """forward_backward with a scaler: grads() are the true (unscaled) gradients; the overflow flag goes to
        found_inf() and is cleared here, since no dbsr_loss_scale_update follows (the state is a step's alone)."""
        if not self.scaling:
            return
        self._unscale_flow_grad(stream)
        L.check(L.lib().dbsr_grad_unscale_check(self.n_params, self.flat_grad.data_ptr(), self._ls.data_ptr(),
                                                stream), 'grad_unscale_check')
        flag = self._ls[L.LS_FOUND_INF:L.LS_FOUND_INF + 1]
        self._fb_inf.copy_(flag)
        flag.zero_()

    def found_inf(self):
        """Whether the last forward_backward's gradients overflowed (copies one int to the host; for tests)."""
        return bool(int(self._fb_inf)) if self.scaling else False

    def loss_scale_state(self):
        """{'scale', 'growth_tracker', 'steps', 'skipped'} of the loss scaler ('steps': optimizer steps applied),
        None without one.  One small device-to-host copy: for logging and tests, never part of a step."""
        if not self.scaling:
            return None
        w = self._ls.cpu()
        return {'scale': float(w.view(torch.float32)[L.LS_SCALE]), 'growth_tracker': int(w[L.LS_GROWTH_TRACKER]),
                'steps': int(w[L.LS_ADAM_STEP]), 'skipped': int(w[L.LS_SKIPPED])}

    def set_loss_scale(self, scale):
        """Overwrite the scaler's current scale (resuming a run; tests)."""
        if not self.scaling:
            raise ValueError('DBSRTrainer: built without a loss scaler')
        self._ls.view(torch.float32)[L.LS_SCALE] = float(scale)

    # ---- autograd through DBSRNet.forward (the reference's own loop: pred, _ = net(burst); objective(pred,
    # gt).backward(); optimizer.step(); actors/dbsr_actors.py:27-47, trainers/simple_trainer.py:78-81) ----
    def _plan(self, shape, flow=None, flow_grad=None):
        """The plan of a burst shape; with external flows a plan of its own (no PWC-Net ops), keyed separately.
        flow_grad: None = the trainer's setting (the autograd path asks per call, by flow.requires_grad)."""
        B, N, _, H, W = shape
        if flow is not None and tuple(flow.shape) != (B, N - 1, 2, H, W):
            raise ValueError('DBSRTrainer: flow must be [B,N-1,2,H,W] = %s, got %s'
                             % ((B, N - 1, 2, H, W), tuple(flow.shape)))
        fg = self.want_flow_grad if flow_grad is None else bool(flow_grad)
        key = (B, N, H, W) if flow is None else (B, N, H, W, 'flow') + ((fg,) if fg != self.want_flow_grad else ())
        plan = self.plans.get(key)
        if plan is None:
            plan = self.plans[key] = self._build(B, N, H, W, ext_flow=flow is not None, flow_grad=fg)
        return plan

    def forward_saved(self, burst, flow=None, flow_grad=None):
        """The training forward with every activation kept in the plan's buffers: (pred, offsets, fusion
        weights, token).  The activations stay valid until the next forward of the same shape; `token`
        names them for backward_from.  flow: the caller's offsets [B,N-1,2,H,W] instead of PWC-Net's."""
        plan = self._load(burst, None, flow, flow_grad)
        plan.run_list(plan.ops[:plan.fwd_end], L.stream_ptr(self.dev))
        plan.gen += 1
        B, N, _, H, W = burst.shape
        fw = plan.FW.t.clone().view(B, N, H, W, -1).permute(0, 1, 4, 2, 3)
        return plan.bufs['pred'].clone(), plan.bufs['offsets'].view(B, N - 1, 2, H, W).clone(), fw, \
            (plan, plan.gen)

    def backward_from(self, token, gpred):
        """Gradients of the DBSR parameters (list in self.params order, fp32) from dL/dpred of the forward
        that returned `token`."""
        plan, gen = token
        if plan.gen != gen:
            raise RuntimeError('DBSRNet training: backward() after another forward of the same burst shape -- the '
                               'saved activations are gone (one forward per backward, as in the reference loop)')
        plan.bufs['gpred'].copy_(gpred.to(torch.float32), non_blocking=True)
        fn, args, name, _ = plan.grad_in_op
        L.check(fn(*args, L.stream_ptr(self.dev)), name)
        plan.run_list(plan.ops[plan.fwd_end + 1:], L.stream_ptr(self.dev))
        self._flow_plan = plan
        return [self.flat_grad[o:o + k].view(p.shape).clone() for p in self.params for (o, k) in [self.offset[id(p)]]]

    def grads(self):
        """{parameter name: gradient} views of the flat gradient buffer."""
        names = {id(p): n for n, p in self.net.named_parameters()}
        return {names[id(p)]: self.flat_grad[o:o + k].view(p.shape) for p in self.params
                for (o, k) in [self.offset[id(p)]]}


class DBSRRealWorldTrainer(DBSRTrainer):
    """The real-world fine-tuning step (train_settings/dbsr/default_realworld.py:65-79 with
    actors/dbsr_actors.py:50-95): DBSRTrainer's step with the L1 objective replaced by the aligned one,

        pred, _ = net(burst); out, valid = sca(pred, gt, burst); loss = loss_weight * L1(out, gt, valid=valid)

    The plan is DBSRTrainer's, op for op: the forward ops[:fwd_end] run, then the alignment segment (no gradient:
    PWC flow pred -> gt, the x1/(2 sr_factor) flow and ground truth, the warped base frame, the two smoothings,
    dbsr_color_fit, the validity mask -- burstsr.SpatialColorAlignment.align), then dbsr_aligned_l1_forward /
    _backward write the loss and the predictor's gated gradient dP in place of the plan's l1_loss_bwd op, then
    ops[fwd_end + 1:], the bucketed all-reduce and Adam as DBSRTrainer.step.  The alignment and the objective
    are fp32 whatever the network's compute dtype; nothing is read back to the host during a step.

    alignment_net: a dbsr_amd PWCNet on the same device (frozen; its own fp32 engine).  After a step / a
    forward_backward: `last_alignment` = (flow, c_mat, valid) and `last_stats` = {'loss', 'psnr'} (the actor's
    Loss/total and Stat/psnr; reading last_stats copies a few floats to the host)."""

    def __init__(self, net, alignment_net, sr_factor=4, loss_weight=10.0, boundary_ignore=40, **kwargs):
        if getattr(net, 'compute_dtype', None) == torch.float16 or kwargs.get('loss_scale') is not None:
            # the aligned objective writes dP itself (dbsr_aligned_l1_backward, in place of the plan's l1_loss_bwd
            # op) and is not scaled yet: refuse before anything is allocated
            raise ValueError('DBSRRealWorldTrainer: train in torch.bfloat16 or torch.float32 (the aligned objective '
                             'has no loss scaling here)')
        if kwargs.get('objective') is not None:
            raise ValueError('DBSRRealWorldTrainer: the step\'s objective is the aligned L1 of the real-world recipe; '
                             'objective= belongs to DBSRTrainer')
        if kwargs.get('alignment_grad'):
            raise NotImplementedError('DBSRRealWorldTrainer: alignment_grad=True is not supported (the real-world '
                                      'step has its own segments; train PWC-Net with DBSRTrainer)')
        super().__init__(net, boundary_ignore=boundary_ignore, **kwargs)
        from .burstsr import SpatialColorAlignment
        if self.s != 2 * sr_factor:
            # flow / 8 must land on the burst's grid (spatial_color_alignment.py:96-103 with the x8 RAW network)
            raise ValueError('DBSRRealWorldTrainer: the network upsamples x%d, the alignment needs x%d (2 * sr_factor)'
                             % (self.s, 2 * sr_factor))
        self.sca = SpatialColorAlignment(alignment_net, sr_factor=sr_factor)
        self.loss_weight = float(loss_weight)
        self._loss2 = torch.zeros(2, dtype=torch.float32, device=self.dev)       # {loss, gradient scale}
        self.loss = self._loss2[:1]
        self.last_alignment = None
        self._stats = None

    def _objective(self, plan, stream):
        """Alignment segment + the aligned L1 forward / backward into plan.dP."""
        lib = L.lib()
        pred, gt = plan.bufs['pred'], plan.bufs['gt']
        B, _, HS, WS = pred.shape
        rw = getattr(plan, 'rw', None)
        if rw is None:
            need = lib.dbsr_aligned_l1_workspace_bytes(B, HS, WS)
            rw = plan.rw = dict(need=need, ws=torch.empty(max(need, 16), dtype=torch.uint8, device=self.dev),
                                g_pw=torch.empty(B, 3, HS, WS, dtype=torch.float32, device=self.dev),
                                stats=torch.zeros(B, 2, dtype=torch.float32, device=self.dev))
        flow, cmat, valid = self.sca.align(pred, gt, plan.bufs['burst'])
        self.last_alignment = (flow, cmat, valid)
        L.check(lib.dbsr_aligned_l1_forward(B, HS, WS, self.bi, pred.data_ptr(), flow.data_ptr(), cmat.data_ptr(),
                                            valid.data_ptr(), gt.data_ptr(), self.loss_weight, rw['g_pw'].data_ptr(),
                                            self._loss2.data_ptr(), rw['stats'].data_ptr(), rw['ws'].data_ptr(),
                                            rw['need'], stream), 'dbsr_aligned_l1_forward')
        L.check(lib.dbsr_aligned_l1_backward(B, HS, WS, pred.data_ptr(), flow.data_ptr(), rw['g_pw'].data_ptr(), None,
                                             self._loss2.data_ptr() + 4, None, plan.dP.d(0), rw['ws'].data_ptr(),
                                             rw['need'], stream), 'dbsr_aligned_l1_backward')
        self._stats = rw['stats']

    @property
    def last_stats(self):
        """{'loss': Loss/total, 'psnr': Stat/psnr} of the last step (dbsr_actors.py:82-93; PSNR(boundary_ignore)
        with the validity mask, images with an infinite / undefined PSNR dropped, image_quality_v2.py:88-101)."""
        if self._stats is None:
            return None
        st = self._stats.double().cpu()
        psnr = [-10.0 * math.log10(sq / (3.0 * n + 1e-12)) for sq, n in st.tolist() if sq > 0.0 and n > 0.0]
        return {'loss': float(self._loss2[0]), 'psnr': sum(psnr) / len(psnr) if psnr else 0}

    def step(self, burst, frame_gt, flow=None):
        """One fine-tuning step on this rank's bursts [B,N,4,H,W] and ground truth [B,3,8H,8W] (flow: as
        DBSRTrainer.step); returns the rank-local loss (device tensor, shape [1])."""
        plan = self._load(burst, frame_gt, flow)
        stream = L.stream_ptr(self.dev)
        fe = plan.fwd_end
        # the forward, [the objective, eager], then the backward cut at the gradient buckets' completion points;
        # each segment of plan ops is one HIP graph replay after one eager step (as DBSRTrainer.step)
        cuts = [fe + 1] + ([b[0] for b in plan.buckets] if self.world > 1 else []) + [len(plan.ops)]
        segs = [(0, fe)] + [(a, b) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]
        if self.use_graph and plan.graphs is None and plan.eager_runs > 0:
            plan.graphs = []
            for a, b in segs:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    plan.run_list(plan.ops[a:b], L.stream_ptr(self.dev))
                plan.graphs.append(g)
        works = []
        bi = 0
        for si, (a, b) in enumerate(segs):
            if plan.graphs is not None:
                plan.graphs[si].replay()
            else:
                plan.run_list(plan.ops[a:b], stream)
            if si == 0:
                self._objective(plan, stream)
            while bi < len(plan.buckets) and plan.buckets[bi][0] == b:
                if self.world > 1:
                    _, lo, hi = plan.buckets[bi]
                    works.append(allreduce_bucket(self.flat_grad, lo, hi, self.pg))
                bi += 1
        plan.eager_runs += 1
        for w_ in works:
            w_.wait()
        self._optimizer_step(stream)
        return self.loss.clone()

    def forward_backward(self, burst, frame_gt, flow=None):
        """Loss and gradients only (no all-reduce, no optimizer step): for tests."""
        plan = self._load(burst, frame_gt, flow)
        stream = L.stream_ptr(self.dev)
        plan.run_list(plan.ops[:plan.fwd_end], stream)
        self._objective(plan, stream)
        plan.run_list(plan.ops[plan.fwd_end + 1:], stream)
        return self.loss, plan.bufs['pred']


def trainable_convs(net):
    """The DBSR convs that train, in the order their gradients complete in the backward (decoder, then
    merging, then encoder); the flat parameter / gradient buffers follow this order (weight, bias)."""
    dec, mer, enc = net.decoder, net.merging, net.encoder
    mods = [dec.predictor[0]]
    for b in reversed(list(dec.post_res_layers)):
        mods += [b.conv2[0], b.conv1[0]]
    mods.append(dec.upsample_layer.conv_layer[0])
    for b in reversed(list(dec.pre_res_layers)):
        mods += [b.conv2[0], b.conv1[0]]
    mods.append(dec.init_layer[0])
    wp = list(mer.weight_predictor)
    mods.append(wp[-1][0])
    for b in reversed(wp[1:-1]):
        mods += [b.conv2[0], b.conv1[0]]
    mods.append(wp[0][0])
    ofe = list(mer.offset_feat_extractor)
    for b in reversed(ofe[1:]):
        mods += [b.conv2[0], b.conv1[0]]
    mods.append(ofe[0][0])
    mods.append(mer.feat_project_layer[0])
    mods.append(enc.out_layer[0])
    for b in reversed(list(enc.res_layers)):
        mods += [b.conv2[0], b.conv1[0]]
    mods.append(enc.init_layer[0])
    return mods


def flat_layout(net):
    """[(parameter name, numel)] of the flat buffers, and the (lo, hi) element ranges of the three
    gradient buckets (decoder, merging, encoder) that the backward completes in that order."""
    names = {id(p): n for n, p in net.named_parameters()}
    layout, bounds, o = [], {}, 0
    for m in trainable_convs(net):
        for p in [m.weight] + ([m.bias] if m.bias is not None else []):
            n = names[id(p)]
            layout.append((n, p.numel()))
            part = n.split('.')[0]
            lo, hi = bounds.get(part, (o, o))
            bounds[part] = (min(lo, o), o + p.numel())
            o += p.numel()
    return layout, [bounds['decoder'], bounds['merging'], bounds['encoder']]


def allreduce_bucket(flat_grad, lo, hi, group=None):
    """Start the sum all-reduce of one gradient bucket (RCCL on HIP tensors, gloo on CPU tensors); the
    caller scales by 1/world (folded into the Adam step)."""
    return dist.all_reduce(flat_grad[lo:hi], group=group, async_op=True)


class _DBSRTrainForward(torch.autograd.Function):
    """DBSRNet.forward under autograd: the HIP training forward (activations saved) and, on backward, the
    HIP backward from dL/dpred into the DBSR parameters' gradients (PWC-Net is frozen, encoders.py:56-61) and,
    with the caller's own `flow`, into that flow (through the warp and the offset-feature extractor)."""

    @staticmethod
    def forward(ctx, burst, engine, flow, *params):
        ctx.flow_grad = flow is not None and flow.requires_grad
        pred, offs, fw, token = engine.forward_saved(burst, flow, ctx.flow_grad if flow is not None else None)
        ctx.engine, ctx.token = engine, token
        ctx.mark_non_differentiable(offs, fw)
        return pred, offs, fw

    @staticmethod
    def backward(ctx, gpred, goffs, gfw):
        if gpred is None:
            return (None, None, None) + tuple(None for _ in ctx.engine.params)
        grads = tuple(ctx.engine.backward_from(ctx.token, gpred.contiguous()))
        gflow = ctx.engine.flow_grad().clone() if ctx.flow_grad else None
        return (None, None, gflow) + grads


def _aliased(eng):
    """Every trained parameter still lives in the trainer's flat buffer (p.data = ..., load_state_dict(assign=True)
    or a device move replace the storage; the trainer would then pack a stale copy)."""
    cur = [p for m in trainable_convs(eng.net) for p in [m.weight] + ([m.bias] if m.bias is not None else [])]
    if len(cur) != len(eng.params) or any(a is not b for a, b in zip(cur, eng.params)):
        return False                                   # new Parameter objects (load_state_dict(assign=True))
    base = eng.flat.data_ptr()
    return all(p.data_ptr() == base + 4 * eng.offset[id(p)][0] and p.device == eng.dev and
               p.dtype == torch.float32 for p in eng.params)


def train_forward(net, burst, flow=None):
    """pred, {'offsets', 'fusion_weights'} of DBSRNet.forward with autograd to the DBSR parameters and, when the
    caller supplies the offsets (flow [B,N-1,2,H,W], e.g. their own alignment network's output), to that flow."""
    eng = getattr(net, '_train_engine', None)
    if eng is None or eng.net is not net or eng.dtype != net.compute_dtype or not _aliased(eng):
        eng = net._train_engine = DBSRTrainer(net, optimizer=False,
                                              alignment_grad=bool(getattr(net.encoder, 'train_alignmentnet', False)))
    pred, offs, fw = _DBSRTrainForward.apply(burst, eng, flow, *eng.params)
    from .engine import DBSRAux
    return pred, DBSRAux(offs, fw)
