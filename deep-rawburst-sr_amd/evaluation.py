"""Evaluation-harness counterpart for the DBSR forward.

The reference's SyntheticBurstVal scoring cannot run on this stack (dataset/synthetic_burst_val_set.py
needs cv2; evaluation/synburst/compute_score.py needs cv2, lpips and torch._six via the dataset
package).  This module restates the parts that decide the reported number, so a user of the reference
can score the drop-in network on the same files:

  * a 16-bit PNG codec with cv2's channel conventions (`imread_unchanged`, `imwrite`): cv2 stores
    arrays as BGR(A), so the on-disk RGB(A) planes are the array's channels in [2,1,0(,3)] order
    (synthetic_burst_val_set.py:43-54 reads with cv2.IMREAD_UNCHANGED; save_results.py:63-67 writes
    with cv2.imwrite).  Pillow is not usable for this: it reduces 16-bit RGB(A) to 8 bits.
  * `SyntheticBurstVal` (synthetic_burst_val_set.py:20-79): bursts/NNNN/im_raw_KK.png (4-channel
    RGGB, /2^14), gt/NNNN/im_rgb.png (3-channel, /2^14).  meta_info.pkl is NOT unpickled here (it is
    only used for sRGB visualisation, which is out of scope); meta_info carries 'burst_name' only.
  * `quantize_prediction` (compute_score.py:109-111) and `PSNR` / `PixelWiseError`
    (models/loss/image_quality_v2.py:24-101), `SSIM` (image_quality_v2.py:104-136 over
    models/loss/msssim.py:10-74), `MSSSIM` (msssim.py:77-103), `compute_score` (compute_score.py:36-122,
    PSNR and SSIM columns, MS-SSIM on request) and `save_results` (save_results.py:36-67).
  * `LPIPS` (image_quality_v2.py:139-163 over the `lpips` package's v0.1 metric, restated), the last column:
    reported when the caller hands over the package's AlexNet / VGG weights and linear heads
    (`compute_score(..., lpips=LPIPS(weights=...))`).  No weights are shipped or downloaded.

Host-side Python only: the network forward is the HIP path; PSNR runs as torch ops on whatever device
the predictions live on; SSIM on device tensors runs the HIP kernels of csrc/metrics.hip (forward and
gradient), on CPU tensors a torch restatement of the reference arithmetic.  MS-SSIM is host-side only: a
torch restatement on CPU tensors.  LPIPS on device tensors runs the HIP plan of ops.LPIPSPlan (csrc/lpips.hip
and the fp32 convs; with differentiable=True also its HIP backward, csrc/lpips_grad.hip), on CPU tensors a torch
restatement.
"""
import math
import os
import struct
import zlib

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

_PNG_SIG = b'\x89PNG\r\n\x1a\n'
_COLOR_CHANNELS = {0: 1, 2: 3, 4: 2, 6: 4}       # PNG colour type -> samples per pixel


# ------------------------------------------------------------------------------------------ PNG codec

def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def png_read(path):
    """Decode a non-interlaced 8/16-bit gray/gray-alpha/RGB/RGBA PNG into an [H,W,C] array holding the
    FILE's channel order (uint8 or uint16).  Raises ValueError on anything else (palette,
    interlace, bit depths < 8), which SyntheticBurstVal/BurstSR files never use."""
    with open(path, 'rb') as f:
        data = f.read()
    if data[:8] != _PNG_SIG:
        raise ValueError(f'{path}: not a PNG file')
    pos, idat, hdr = 8, [], None
    while pos < len(data):
        ln, typ = struct.unpack('>I4s', data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + ln]
        if zlib.crc32(typ + body) & 0xffffffff != struct.unpack('>I', data[pos + 8 + ln:pos + 12 + ln])[0]:
            raise ValueError(f'{path}: CRC mismatch in {typ!r} chunk')
        if typ == b'IHDR':
            hdr = struct.unpack('>IIBBBBB', body)
        elif typ == b'IDAT':
            idat.append(body)
        elif typ == b'IEND':
            break
        pos += 12 + ln
    if hdr is None:
        raise ValueError(f'{path}: missing IHDR')
    w, h, depth, ctype, _, _, interlace = hdr
    if depth not in (8, 16) or ctype not in _COLOR_CHANNELS or interlace != 0:
        raise ValueError(f'{path}: unsupported PNG (depth {depth}, colour type {ctype}, interlace {interlace})')
    ch = _COLOR_CHANNELS[ctype]
    bpp = ch * depth // 8
    stride = w * bpp
    raw = np.frombuffer(zlib.decompress(b''.join(idat)), dtype=np.uint8)
    if raw.size != h * (stride + 1):
        raise ValueError(f'{path}: image data size {raw.size} != {h}*({stride}+1)')
    rows = raw.reshape(h, stride + 1)
    out = np.zeros((h, stride), dtype=np.uint8)
    prev = np.zeros(stride, dtype=np.int32)
    for y in range(h):
        ft, line = rows[y, 0], rows[y, 1:].astype(np.int32)
        if ft == 0:
            cur = line
        elif ft == 1:     # Sub: running sum along the row, per byte lane of a pixel
            cur = np.cumsum(line.reshape(w, bpp), axis=0).reshape(-1) & 0xff
        elif ft == 2:     # Up
            cur = (line + prev) & 0xff
        elif ft in (3, 4):  # Average / Paeth: sequential along the row, vectorised over the pixel's bytes
            cur = np.empty(stride, dtype=np.int32)
            left = np.zeros(bpp, dtype=np.int32)
            upleft = np.zeros(bpp, dtype=np.int32)
            for x in range(0, stride, bpp):
                up = prev[x:x + bpp]
                pred = (left + up) >> 1 if ft == 3 else _paeth(left, up, upleft)
                left = (line[x:x + bpp] + pred) & 0xff
                cur[x:x + bpp] = left
                upleft = up
        else:
            raise ValueError(f'{path}: bad filter type {ft} in row {y}')
        out[y] = cur
        prev = cur
    if depth == 16:
        return out.view('>u2').astype(np.uint16).reshape(h, w, ch)
    return out.reshape(h, w, ch)


def png_write(path, img, filter_type=0, level=6):
    """Encode an [H,W] or [H,W,C] uint8/uint16 array (FILE channel order, C in 1..4) as a PNG.
    `filter_type` 0..4 applies that filter to every row (tests use it to cover the decoder)."""
    img = np.ascontiguousarray(img)
    if img.ndim == 2:
        img = img[:, :, None]
    h, w, ch = img.shape
    if img.dtype == np.uint16:
        depth, buf = 16, img.astype('>u2').view(np.uint8)
    elif img.dtype == np.uint8:
        depth, buf = 8, img
    else:
        raise ValueError(f'png_write: dtype {img.dtype} (want uint8 or uint16)')
    ctype = {1: 0, 2: 4, 3: 2, 4: 6}[ch]
    bpp = ch * depth // 8
    cur = buf.reshape(h, w * bpp).astype(np.int32)
    up = np.vstack([np.zeros((1, w * bpp), np.int32), cur[:-1]])
    left = np.hstack([np.zeros((h, bpp), np.int32), cur[:, :-bpp]])
    upleft = np.hstack([np.zeros((h, bpp), np.int32), up[:, :-bpp]])
    pred = {0: 0, 1: left, 2: up, 3: (left + up) >> 1, 4: _paeth(left, up, upleft)}[filter_type]
    filt = ((cur - pred) & 0xff).astype(np.uint8)
    raw = np.hstack([np.full((h, 1), filter_type, np.uint8), filt]).tobytes()

    def chunk(typ, body):
        return struct.pack('>I', len(body)) + typ + body + struct.pack('>I', zlib.crc32(typ + body) & 0xffffffff)
    with open(path, 'wb') as f:
        f.write(_PNG_SIG + chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, depth, ctype, 0, 0, 0))
                + chunk(b'IDAT', zlib.compress(raw, level)) + chunk(b'IEND', b''))


def _bgr_order(ch):
    return [2, 1, 0, 3][:ch] if ch >= 3 else list(range(ch))


def imread_unchanged(path):
    """cv2.imread(path, cv2.IMREAD_UNCHANGED): [H,W] for gray, else [H,W,C] in BGR(A) order."""
    img = png_read(path)
    if img.shape[2] == 1:
        return img[:, :, 0]
    return np.ascontiguousarray(img[:, :, _bgr_order(img.shape[2])])


def imwrite(path, img):
    """cv2.imwrite(path, img) for PNG: the array is BGR(A), the file stores RGB(A)."""
    img = np.asarray(img)
    if img.ndim == 3 and img.shape[2] >= 3:
        img = img[:, :, _bgr_order(img.shape[2])]
    png_write(path, img)


# ------------------------------------------------------------------------------------------ dataset

class SyntheticBurstVal(torch.utils.data.Dataset):
    """dataset/synthetic_burst_val_set.py:20-79 (cv2 replaced by `imread_unchanged`)."""

    def __init__(self, root, initialize=True, burst_size=14, num_bursts=None):
        self.root = root
        if num_bursts is None:   # the reference hard-codes 300 (:32); count what is on disk instead
            bdir = os.path.join(root, 'bursts')
            num_bursts = len([d for d in os.listdir(bdir) if d.isdigit()]) if os.path.isdir(bdir) else 300
        self.burst_list = list(range(num_bursts))
        self.burst_size = burst_size

    def initialize(self):
        pass

    def __len__(self):
        return len(self.burst_list)

    def _read_burst_image(self, index, image_id):
        im = imread_unchanged('{}/bursts/{:04d}/im_raw_{:02d}.png'.format(self.root, index, image_id))
        return torch.from_numpy(im.astype(np.float32)).permute(2, 0, 1).float() / (2 ** 14)

    def _read_gt_image(self, index):
        gt = imread_unchanged('{}/gt/{:04d}/im_rgb.png'.format(self.root, index))
        return (torch.from_numpy(gt.astype(np.float32)) / 2 ** 14).permute(2, 0, 1).float()

    def __getitem__(self, index):
        burst = torch.stack([self._read_burst_image(index, i) for i in range(self.burst_size)], 0)
        gt = self._read_gt_image(index)
        return burst, gt, {'burst_name': '{:04d}'.format(index)}


def write_synthetic_burst_val(root, bursts, gts, start=0):
    """Write bursts [B,N,4,H,W] and gts [B,3,sH,sW] (values in [0,1]) in the SyntheticBurstVal layout,
    quantised to 2^14 the way the dataset's PNGs are.  Used to exercise the reader and the scorer
    without the (unavailable) dataset."""
    for b in range(bursts.shape[0]):
        name = '{:04d}'.format(start + b)
        os.makedirs(os.path.join(root, 'bursts', name), exist_ok=True)
        os.makedirs(os.path.join(root, 'gt', name), exist_ok=True)
        for i in range(bursts.shape[1]):
            im = (bursts[b, i].permute(1, 2, 0).clamp(0, 1) * 2 ** 14).round().numpy().astype(np.uint16)
            imwrite(os.path.join(root, 'bursts', name, 'im_raw_{:02d}.png'.format(i)), im)
        gt = (gts[b].permute(1, 2, 0).clamp(0, 1) * 2 ** 14).round().numpy().astype(np.uint16)
        imwrite(os.path.join(root, 'gt', name, 'im_rgb.png'), gt)


# ------------------------------------------------------------------------------------------ metrics

def quantize_prediction(pred):
    """compute_score.py:109-111: (clamp(0,1)*2^14).short() / 2^14."""
    return (pred.clamp(0.0, 1.0) * 2 ** 14).short().float() / (2 ** 14)


class PixelWiseError(nn.Module):
    """models/loss/image_quality_v2.py:24-66."""

    def __init__(self, metric='l1', boundary_ignore=None):
        super().__init__()
        self.boundary_ignore = boundary_ignore
        if metric == 'l1':
            self.loss_fn = F.l1_loss
        elif metric == 'l2':
            self.loss_fn = F.mse_loss
        elif metric == 'l2_sqrt':
            self.loss_fn = lambda pred, gt: (((pred - gt) ** 2).sum(dim=-3)).sqrt().mean()
        elif metric == 'charbonnier':
            self.loss_fn = lambda pred, gt: ((pred - gt) ** 2 + 1e-3 ** 2).sqrt().mean()
        else:
            raise ValueError(f'unknown metric {metric!r}')

    def forward(self, pred, gt, valid=None):
        if self.boundary_ignore is not None:
            bi = self.boundary_ignore
            pred = pred[..., bi:-bi, bi:-bi]
            gt = gt[..., bi:-bi, bi:-bi]
            if valid is not None:
                valid = valid[..., bi:-bi, bi:-bi]
        if valid is None:
            return self.loss_fn(pred, gt)
        err = self.loss_fn(pred, gt, reduction='none')
        elem_ratio = err.numel() / valid.numel()
        return (err * valid.float()).sum() / (valid.float().sum() * elem_ratio + 1e-12)


class PSNR(nn.Module):
    """models/loss/image_quality_v2.py:69-101: per-image PSNR, inf/nan images dropped, then the mean."""

    def __init__(self, boundary_ignore=None, max_value=1.0):
        super().__init__()
        self.l2 = PixelWiseError(metric='l2', boundary_ignore=boundary_ignore)
        self.max_value = max_value

    def psnr(self, pred, gt, valid=None):
        mse = self.l2(pred, gt, valid=valid)
        if self.max_value is not None:
            return 20 * math.log10(self.max_value) - 10.0 * mse.log10()
        return 20 * gt.max().log10() - 10.0 * mse.log10()

    def forward(self, pred, gt, valid=None):
        if valid is None:
            vals = [self.psnr(p.unsqueeze(0), g.unsqueeze(0)) for p, g in zip(pred, gt)]
        else:
            vals = [self.psnr(p.unsqueeze(0), g.unsqueeze(0), v.unsqueeze(0)) for p, g, v in zip(pred, gt, valid)]
        vals = [p for p in vals if not (torch.isinf(p) or torch.isnan(p))]
        return 0 if not vals else sum(vals) / len(vals)


def _ssim_window(channel, like):
    """msssim.gaussian / create_window: 11 taps of exp(-(x-5)^2 / (2 * 1.5^2)) as float32 over their sum,
    the float32 outer product, one copy per channel, then cast to the images' dtype."""
    g = torch.tensor([math.exp(-(x - 5) ** 2 / float(2 * 1.5 ** 2)) for x in range(11)], dtype=torch.float32)
    g = (g / g.sum()).unsqueeze(1)
    w = g.mm(g.t()).float().expand(channel, 1, 11, 11).contiguous()
    return w.to(device=like.device, dtype=like.dtype)


def ssim_val_range(img):
    """msssim.py:24-34: the dynamic range the reference infers when none is given (max > 128 -> 255 else 1,
    min < -0.5 -> -1 else 0).  One host read."""
    lo, hi = torch.aminmax(img.detach())
    return (255 if float(hi) > 128 else 1) - (-1 if float(lo) < -0.5 else 0)


def ssim_map(pred, gt, val_range):
    """msssim.py:45-63 with the 11x11 window: the SSIM map [B, C, H-10, W-10] of [B, C, H, W] images, as
    torch ops in the images' dtype (the CPU path of `SSIM`, and the oracle of the HIP kernels)."""
    ch = pred.shape[1]
    win = _ssim_window(ch, pred)
    filt = lambda t: F.conv2d(t, win, padding=0, groups=ch)                              # noqa: E731
    mu1, mu2 = filt(pred), filt(gt)
    mu1_sq, mu2_sq, mu12 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s11 = filt(pred * pred) - mu1_sq
    s22 = filt(gt * gt) - mu2_sq
    s12 = filt(pred * gt) - mu12
    c1, c2 = (0.01 * val_range) ** 2, (0.03 * val_range) ** 2
    return ((2 * mu12 + c1) * (2.0 * s12 + c2)) / ((mu1_sq + mu2_sq + c1) * (s11 + s22 + c2))


class _SSIMHip(torch.autograd.Function):
    """Masked mean SSIM on the HIP kernels (ops.ssim_forward / ssim_backward), with autograd to pred."""

    @staticmethod
    def forward(ctx, pred, gt, valid, bi, val_range):
        from . import ops
        in_dtype = pred.dtype
        pred, gt = pred.detach().float().contiguous(), gt.detach().float().contiguous()
        valid = None if valid is None else valid.to(torch.uint8).contiguous()
        result, _, _ = ops.ssim_forward(pred, gt, valid, bi, val_range)
        ctx.save_for_backward(pred, gt, result, *(() if valid is None else (valid,)))
        ctx.bi, ctx.val_range, ctx.in_dtype = bi, val_range, in_dtype
        return result[0].clone()

    @staticmethod
    def backward(ctx, gout):
        from . import ops
        pred, gt, result = ctx.saved_tensors[:3]
        valid = ctx.saved_tensors[3] if len(ctx.saved_tensors) > 3 else None
        gpred = ops.ssim_backward(pred, gt, valid, ctx.bi, ctx.val_range, scale=result[1:] * gout.float())
        return gpred.to(ctx.in_dtype), None, None, None, None


class SSIM(nn.Module):
    """models/loss/image_quality_v2.py:104-136: the mean (or, with `valid`, the masked mean) of the SSIM map
    inside the boundary crop; 1 - ssim when `use_for_loss`.  `val_range=None` applies the reference's
    data-dependent rule to the cropped prediction (one host read); a number skips the read.  Device tensors
    run the HIP kernels (gradient to pred); CPU tensors the torch restatement `ssim_map`."""

    def __init__(self, boundary_ignore=None, use_for_loss=True, val_range=None):
        super().__init__()
        self.boundary_ignore = boundary_ignore
        self.use_for_loss = use_for_loss
        self.val_range = val_range

    def forward(self, pred, gt, valid=None):
        if pred.dim() == 3:
            pred, gt = pred.unsqueeze(0), gt.unsqueeze(0)
            if valid is not None and valid.dim() == 3:
                valid = valid.unsqueeze(0)
        bi = self.boundary_ignore or 0
        crop = (lambda t: t[..., bi:-bi, bi:-bi]) if bi else (lambda t: t)
        val_range = self.val_range if self.val_range is not None else ssim_val_range(crop(pred))
        if pred.is_cuda:
            value = _SSIMHip.apply(pred, gt, valid, bi, float(val_range))
        else:
            smap = ssim_map(crop(pred), crop(gt), val_range)
            if valid is not None:
                v = crop(valid)[..., 5:-5, 5:-5].to(smap.dtype)          # window centres (window size 11)
                elem_ratio = smap.numel() / v.numel()
                value = (smap * v).sum() / (v.sum() * elem_ratio + 1e-12)
            else:
                value = smap.mean()
        return 1.0 - value if self.use_for_loss else value


# ------------------------------------------------------------------------------------------ MS-SSIM

MSSSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)       # msssim.py:79, held as float32
MSSSIM_MIN_SIDE = 32                                             # the reference pools a fifth time (msssim.py:88)


def _gauss_window(k, channel, like):
    """msssim.gaussian(k, 1.5) / create_window: k taps of exp(-(x - k//2)^2 / (2 * 1.5^2)) as float32 over their sum
    (off-centre for even k), the float32 outer product, one copy per channel, then cast to the images' dtype as
    msssim.SSIM.forward does."""
    g = torch.tensor([math.exp(-(x - k // 2) ** 2 / float(2 * 1.5 ** 2)) for x in range(k)], dtype=torch.float32)
    g = (g / g.sum()).unsqueeze(1)
    w = g.mm(g.t()).float().expand(channel, 1, k, k).contiguous()
    return w.to(device=like.device, dtype=like.dtype)


def msssim_levels(pred, gt, val_range):
    """msssim.py:83-89 on already cropped [B, C, H, W] images: the five (s_l, cs_l) = (mean SSIM map, mean
    contrast-structure map) over batch, channels and windows, level l + 1 being F.avg_pool2d(level l, (2, 2)) and
    the window min(11, H_l, W_l) wide.  Torch ops in the images' dtype: what `MSSSIM` computes.  One `val_range`
    serves all five levels (see `MSSSIM`)."""
    if pred.dim() != 4 or min(pred.shape[-2:]) < MSSSIM_MIN_SIDE:
        raise ValueError('msssim: the crop %s is smaller than 32 x 32 (five levels, each pooled by two)'
                         % 'x'.join(str(v) for v in pred.shape[-2:]))
    ch = pred.shape[1]
    c1, c2 = (0.01 * val_range) ** 2, (0.03 * val_range) ** 2
    out = []
    for level in range(len(MSSSIM_WEIGHTS)):
        if level:
            pred, gt = F.avg_pool2d(pred, (2, 2)), F.avg_pool2d(gt, (2, 2))
        win = _gauss_window(min(11, pred.shape[-2], pred.shape[-1]), ch, pred)
        filt = lambda t: F.conv2d(t, win, padding=0, groups=ch)                          # noqa: E731
        mu1, mu2 = filt(pred), filt(gt)
        mu1_sq, mu2_sq, mu12 = mu1.pow(2), mu2.pow(2), mu1 * mu2
        s11 = filt(pred * pred) - mu1_sq
        s22 = filt(gt * gt) - mu2_sq
        s12 = filt(pred * gt) - mu12
        v1, v2 = 2.0 * s12 + c2, s11 + s22 + c2
        cs = torch.mean(v1 / v2)
        out.append((((2 * mu12 + c1) * v1 / ((mu1_sq + mu2_sq + c1) * v2)).mean(), cs))
    return out


def msssim_product(levels, normalize=False, product='reference'):
    """msssim.py:91-103 from the five (s_l, cs_l): 'reference' is torch.prod(pow1[:-1] * pow2[-1]) as it evaluates,
    (prod_{l<4} cs_l^w_l) * s_4^(4 w_4); 'wang2003' uses the exponent w_4 and differs in nothing else."""
    if product not in ('reference', 'wang2003'):
        raise ValueError("msssim: product must be 'reference' or 'wang2003', not %r" % (product,))
    mssim, mcs = torch.stack([s for s, _ in levels]), torch.stack([c for _, c in levels])
    weights = torch.tensor(MSSSIM_WEIGHTS, dtype=torch.float32, device=mssim.device)
    if normalize:
        mssim, mcs = (mssim + 1) / 2, (mcs + 1) / 2
    pow1, pow2 = mcs ** weights, mssim ** weights
    if product == 'reference':
        return torch.prod(pow1[:-1] * pow2[-1])
    return torch.prod(pow1[:-1]) * pow2[-1]


class MSSSIM(nn.Module):
    """models/loss/msssim.py:77-103 (`msssim.msssim`) inside the boundary crop; 1 - value when `use_for_loss`.

    `product='reference'` is the reference's line 102 as it evaluates (the last level's SSIM enters four times);
    `product='wang2003'` uses the exponent w_4 instead of 4 w_4 and differs in nothing else.  `normalize` is the
    reference's (x + 1) / 2.  Without it a negative cs_l gives NaN, as in the reference.  `per_image` scores each
    image as its own B = 1 call and returns [B] (the reference's size_average=False is broken for B > 1 and is not
    offered).  There is no `valid` mask: the reference has no masked MS-SSIM and no mask survives the pooling.
    Crops under 32 x 32 raise ValueError (the reference fails on them).

    `val_range=None` applies `ssim_val_range` to the cropped prediction once (one host read) and uses that range at
    all five levels.  The reference re-derives it per level from the pooled prediction; the two differ only if the
    crop's max exceeds 128 while a pooled level's does not (or likewise for min and -0.5).

    A host-side metric: CPU tensors run the torch restatement `msssim_levels` (differentiable by autograd); device
    tensors raise NotImplementedError, because there is no HIP kernel for it yet and no torch fall-back on the
    device.  `compute_score` copies each quantised prediction to the host for this column."""

    def __init__(self, boundary_ignore=None, use_for_loss=False, val_range=None, normalize=False,
                 product='reference', per_image=False):
        super().__init__()
        if product not in ('reference', 'wang2003'):
            raise ValueError("msssim: product must be 'reference' or 'wang2003', not %r" % (product,))
        self.boundary_ignore = boundary_ignore
        self.use_for_loss = use_for_loss
        self.val_range = val_range
        self.normalize = normalize
        self.product = product
        self.per_image = per_image

    def forward(self, pred, gt):
        if pred.dim() == 3:
            pred, gt = pred.unsqueeze(0), gt.unsqueeze(0)
        bi = self.boundary_ignore or 0
        crop = (lambda t: t[..., bi:-bi, bi:-bi]) if bi else (lambda t: t)
        if min(crop(pred).shape[-2:]) < MSSSIM_MIN_SIDE:
            raise ValueError('msssim: the crop %s is smaller than 32 x 32 (five levels, each pooled by two)'
                             % 'x'.join(str(v) for v in crop(pred).shape[-2:]))
        if pred.is_cuda or gt.is_cuda:
            raise NotImplementedError('MSSSIM is a host-side metric: there is no HIP kernel for it yet and it does '
                                      'not fall back to torch on the device; pass CPU tensors (pred.cpu())')
        val_range = self.val_range if self.val_range is not None else ssim_val_range(crop(pred))
        one = lambda p, g: msssim_product(msssim_levels(crop(p), crop(g), val_range), self.normalize,  # noqa: E731
                                          self.product)
        if self.per_image:
            value = torch.stack([one(pred[i:i + 1], gt[i:i + 1]) for i in range(pred.shape[0])])
        else:
            value = one(pred, gt)
        return 1.0 - value if self.use_for_loss else value


# ------------------------------------------------------------------------------------------ LPIPS
#
# image_quality_v2.LPIPS (:139-163) calls lpips.LPIPS(net)(pred, gt) with the package's normalize=False on [0, 1]
# images.  The package is neither in the reference tree nor installed; what follows restates its published v0.1
# code ('LPIPS').  Weights come from the caller: none are shipped and none are downloaded.

LPIPS_SHIFT = (-.030, -.088, -.188)
LPIPS_SCALE = (.458, .448, .450)
LPIPS_EPS = 1e-10
# per net: the convs (cin, cout, k, stride, pad), the torchvision `features` index of each, the package's slice
# (1..5) each sits in, the program (conv index | 'tap' | ('pool', k, s)) and the smallest crop side
LPIPS_NETS = {
    'alex': dict(
        convs=[(3, 64, 11, 4, 2), (64, 192, 5, 1, 2), (192, 384, 3, 1, 1), (384, 256, 3, 1, 1), (256, 256, 3, 1, 1)],
        features=[0, 3, 6, 8, 10], slices=[1, 2, 3, 4, 5],
        program=[0, 'tap', ('pool', 3, 2), 1, 'tap', ('pool', 3, 2), 2, 'tap', 3, 'tap', 4, 'tap'],
        min_side=31),       # conv1 gives (n - 7) // 4 + 1, the pools (m - 3) // 2 + 1: the second pool needs n >= 31
    'vgg': dict(
        convs=[(3, 64, 3, 1, 1), (64, 64, 3, 1, 1), (64, 128, 3, 1, 1), (128, 128, 3, 1, 1), (128, 256, 3, 1, 1),
               (256, 256, 3, 1, 1), (256, 256, 3, 1, 1), (256, 512, 3, 1, 1), (512, 512, 3, 1, 1),
               (512, 512, 3, 1, 1), (512, 512, 3, 1, 1), (512, 512, 3, 1, 1), (512, 512, 3, 1, 1)],
        features=[0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28], slices=[1, 1, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5, 5],
        program=[0, 1, 'tap', ('pool', 2, 2), 2, 3, 'tap', ('pool', 2, 2), 4, 5, 6, 'tap', ('pool', 2, 2), 7, 8, 9,
                 'tap', ('pool', 2, 2), 10, 11, 12, 'tap'],
        min_side=16),       # four 2 x 2 pools, each m // 2: the fourth needs n >= 16
}


def lpips_tap_channels(net):
    """The channel counts of the five tapped layers."""
    spec, out, last = LPIPS_NETS[net], [], None
    for op in spec['program']:
        if isinstance(op, int):
            last = spec['convs'][op][1]
        elif op == 'tap':
            out.append(last)
    return out


def lpips_state_dict_shapes(net):
    """Key -> shape of the package's LPIPS.state_dict() layout, in the order `generate_lpips_state_dict` documents:
    the backbone convs in network order (weight, then bias), then the five heads."""
    spec = _lpips_spec(net)
    shapes = {}
    for (cin, cout, k, _, _), fi, sl in zip(spec['convs'], spec['features'], spec['slices']):
        shapes['net.slice%d.%d.weight' % (sl, fi)] = (cout, cin, k, k)
        shapes['net.slice%d.%d.bias' % (sl, fi)] = (cout,)
    for l, c in enumerate(lpips_tap_channels(net)):
        shapes['lin%d.model.1.weight' % l] = (1, c, 1, 1)
    return shapes


def generate_lpips_state_dict(net='alex', seed=0):
    """Seeded stand-in weights in the package's state_dict layout, for tests and benchmarks (NOT the trained
    metric).  Like weights.generate_state_dict, each tensor is drawn from its own numpy PCG64 stream seeded with
    [seed, crc32(key)], so the values do not depend on the order of generation; the keys are those of
    `lpips_state_dict_shapes`.  Conv weights are uniform in +-sqrt(6 / fan_in) (activations keep their scale
    through thirteen ReLU layers), biases uniform in +-0.1, heads uniform in [0, 2 / C): non-negative, like the
    trained ones.  Returns float32 torch tensors."""
    out = {}
    for key, shp in lpips_state_dict_shapes(net).items():
        rng = np.random.Generator(np.random.PCG64([int(seed), zlib.crc32(key.encode())]))
        if key.startswith('lin'):
            arr = rng.uniform(0.0, 2.0 / shp[1], size=shp)
        elif key.endswith('.bias'):
            arr = rng.uniform(-0.1, 0.1, size=shp)
        else:
            bound = math.sqrt(6.0 / (shp[1] * shp[2] * shp[3]))
            arr = rng.uniform(-bound, bound, size=shp)
        out[key] = torch.from_numpy(arr.astype(np.float32))
    return out


def _lpips_spec(net):
    if net not in LPIPS_NETS:
        raise ValueError("lpips: type must be 'alex' or 'vgg', not %r" % (net,))
    return LPIPS_NETS[net]


def _lpips_file(src):
    return torch.load(src, map_location='cpu', weights_only=True) if isinstance(src, (str, os.PathLike)) else src


def load_lpips_weights(weights, net='alex', heads=None):
    """Caller-supplied LPIPS weights -> {'net', 'conv_w': [...], 'conv_b': [...], 'lin': [5 x [C]]} of float32 CPU
    tensors.  `weights` (and `heads`) may be a file path (read with torch.load(weights_only=True)) or the object:

      (a) the package's LPIPS.state_dict(): net.slice{1..5}.{i}.weight|bias with i the torchvision `features`
          index, lin{0..4}.model.1.weight [1, C, 1, 1] (duplicates under lins.{l}.model.1.weight are accepted),
          optional scaling_layer.shift|scale (which must hold the v0.1 constants the kernels use);
      (b) a torchvision backbone state_dict (features.{i}.weight|bias; classifier.* is ignored) with the package's
          head file as `heads` (lin{l}.model.1.weight);
      (c) a tuple (conv_weights, conv_biases, lins) of lists of tensors in network order.

    Every shape is validated; every missing or unexpected key is named in the ValueError."""
    spec = _lpips_spec(net)
    chans = lpips_tap_channels(net)
    weights, heads = _lpips_file(weights), _lpips_file(heads)
    problems = []
    if isinstance(weights, (tuple, list)):
        if len(weights) != 3 or heads is not None:
            raise ValueError('lpips weights: the list layout is (conv_weights, conv_biases, lins), without `heads`')
        cw, cb, lins = (list(v) for v in weights)
        if (len(cw), len(cb), len(lins)) != (len(spec['convs']), len(spec['convs']), 5):
            raise ValueError('lpips weights (%s): expected %d conv weights, %d conv biases and 5 heads, got %d, %d, %d'
                             % (net, len(spec['convs']), len(spec['convs']), len(cw), len(cb), len(lins)))
        names = (['conv_weights[%d]' % i for i in range(len(cw))], ['conv_biases[%d]' % i for i in range(len(cb))],
                 ['lins[%d]' % i for i in range(5)])
    elif isinstance(weights, dict):
        sd = dict(weights)
        if heads is not None:
            if not isinstance(heads, dict):
                raise ValueError('lpips weights: `heads` must be a state_dict (lin{l}.model.1.weight)')
            sd.update(heads)
        torchvision = any(k.startswith('features.') for k in sd)
        wk = [('features.%d' % fi) if torchvision else ('net.slice%d.%d' % (sl, fi))
              for fi, sl in zip(spec['features'], spec['slices'])]
        names = ([k + '.weight' for k in wk], [k + '.bias' for k in wk], [])
        for l in range(5):
            k = 'lin%d.model.1.weight' % l
            names[2].append(k if k in sd or ('lins.%d.model.1.weight' % l) not in sd else 'lins.%d.model.1.weight' % l)
        known = set(names[0]) | set(names[1]) | set(names[2])
        known |= {'lin%d.model.1.weight' % l for l in range(5)} | {'lins.%d.model.1.weight' % l for l in range(5)}
        known |= {'scaling_layer.shift', 'scaling_layer.scale'}
        extra = sorted(k for k in sd if k not in known and not (torchvision and k.startswith('classifier.')))
        missing = [k for group in names for k in group if k not in sd]
        if missing:
            problems.append('missing keys %s' % missing)
        if extra:
            problems.append('unexpected keys %s' % extra)
        for key, ref in (('scaling_layer.shift', LPIPS_SHIFT), ('scaling_layer.scale', LPIPS_SCALE)):
            if key in sd:
                t = torch.as_tensor(sd[key]).detach().float().reshape(-1)
                if t.numel() != 3 or not torch.equal(t, torch.tensor(ref, dtype=torch.float32)):
                    problems.append('%s %s is not the v0.1 constant %s' % (key, t.tolist(), list(ref)))
        if problems:
            raise ValueError('lpips weights (%s): %s' % (net, '; '.join(problems)))
        cw, cb, lins = ([sd[k] for k in group] for group in names)
    else:
        raise ValueError('lpips weights: expected a state_dict, a (conv_weights, conv_biases, lins) tuple or a file '
                         'path, not %s' % type(weights).__name__)
    out = {'net': net, 'conv_w': [], 'conv_b': [], 'lin': []}
    for i, (cin, cout, k, _, _) in enumerate(spec['convs']):
        w, b = torch.as_tensor(cw[i]).detach(), torch.as_tensor(cb[i]).detach()
        if tuple(w.shape) != (cout, cin, k, k):
            problems.append('%s has shape %s, expected %s' % (names[0][i], tuple(w.shape), (cout, cin, k, k)))
        if tuple(b.shape) != (cout,):
            problems.append('%s has shape %s, expected %s' % (names[1][i], tuple(b.shape), (cout,)))
        out['conv_w'].append(w.float().cpu().contiguous())
        out['conv_b'].append(b.float().cpu().contiguous())
    for l, c in enumerate(chans):
        v = torch.as_tensor(lins[l]).detach()
        if tuple(v.shape) not in ((1, c, 1, 1), (c,)):
            problems.append('%s has shape %s, expected %s' % (names[2][l], tuple(v.shape), (1, c, 1, 1)))
        out['lin'].append(v.float().cpu().reshape(-1).contiguous())
    if problems:
        raise ValueError('lpips weights (%s): %s' % (net, '; '.join(problems)))
    return out


def lpips_prepare(pred, gt, boundary_ignore=None, bgr2rgb=False):
    """image_quality_v2.LPIPS.forward :153-159: the channel flip, then the boundary crop."""
    if bgr2rgb:
        pred, gt = pred[..., [2, 1, 0], :, :].contiguous(), gt[..., [2, 1, 0], :, :].contiguous()
    bi = boundary_ignore or 0
    if bi:
        pred, gt = pred[..., bi:-bi, bi:-bi], gt[..., bi:-bi, bi:-bi]
    return pred, gt


def _lpips_check_crop(net, h, w):
    need = _lpips_spec(net)['min_side']
    if h < need or w < need:
        raise ValueError('lpips (%s): the crop %d x %d is smaller than %d x %d (the last pool needs a row)'
                         % (net, h, w, need, need))


def lpips_features(x, weights, normalize=False):
    """The five tapped ReLU outputs of the backbone for [N, 3, H, W] images (already flipped and cropped), after
    the optional 2x - 1 and the scaling layer (x - shift) / scale.  Torch ops in x's dtype; the float32 constants
    are cast up as type promotion does in the package."""
    spec = _lpips_spec(weights['net'])
    _lpips_check_crop(weights['net'], x.shape[-2], x.shape[-1])
    if normalize:
        x = 2 * x - 1
    shift = torch.tensor(LPIPS_SHIFT, dtype=torch.float32).to(device=x.device, dtype=x.dtype).view(1, 3, 1, 1)
    scale = torch.tensor(LPIPS_SCALE, dtype=torch.float32).to(device=x.device, dtype=x.dtype).view(1, 3, 1, 1)
    x = (x - shift) / scale
    taps = []
    for op in spec['program']:
        if isinstance(op, int):
            _, _, _, s, p = spec['convs'][op]
            x = F.relu(F.conv2d(x, weights['conv_w'][op].to(x), weights['conv_b'][op].to(x), stride=s, padding=p))
        elif op == 'tap':
            taps.append(x)
        else:
            x = F.max_pool2d(x, op[1], op[2])
    return taps


def lpips_layer_map(f0, f1, lin):
    """d[b, y, x] = sum_c lin[c] (n(f0) - n(f1))^2 with n(f) = f / (sqrt(sum_c f^2) + 1e-10), for [B, C, h, w]."""
    n0 = f0 / (f0.pow(2).sum(dim=1, keepdim=True).sqrt() + LPIPS_EPS)
    n1 = f1 / (f1.pow(2).sum(dim=1, keepdim=True).sqrt() + LPIPS_EPS)
    return ((n0 - n1).pow(2) * lin.to(f0).view(1, -1, 1, 1)).sum(dim=1)


def lpips_maps(pred, gt, weights, normalize=False):
    """The five per-layer distance maps [B, h_l, w_l] of already flipped and cropped [B, 3, H, W] images; both
    images go through the backbone as one batch."""
    B = pred.shape[0]
    taps = lpips_features(torch.cat([pred, gt], 0), weights, normalize)
    return [lpips_layer_map(f[:B], f[B:], lin) for f, lin in zip(taps, weights['lin'])]


def lpips_value(pred, gt, weights, normalize=False):
    """(value [B], per_layer [B, 5], maps): per_layer is each map's mean over y, x; value their sum in layer order."""
    maps = lpips_maps(pred, gt, weights, normalize)
    per_layer = torch.stack([m.mean(dim=(1, 2)) for m in maps], 1)
    value = per_layer[:, 0]
    for l in range(1, 5):
        value = value + per_layer[:, l]
    return value, per_layer, maps


def lpips_layer_grad(f0, f1, lin, gmap):
    """The closed form dbsr_lpips_layer_backward computes, in f0's dtype: d(sum gmap * lpips_layer_map(f0, f1, lin))
    / d f0 for [B, C, h, w] features and gmap [B, h, w] (or broadcastable).  With r = |f0|, D = r + eps, u = f0 / r
    and g = 2 gmap lin (f0 / D - n(f1)): (g - u (u . g) r / D) / D.  At f0 = 0, u = 0: the limit g / eps
    (dn/df = I / eps), which a finite difference confirms and where autograd gives NaN."""
    r = f0.pow(2).sum(dim=1, keepdim=True).sqrt()
    D = r + LPIPS_EPS
    n1 = f1 / (f1.pow(2).sum(dim=1, keepdim=True).sqrt() + LPIPS_EPS)
    g = 2 * gmap.to(f0).reshape(f0.shape[0], 1, *f0.shape[2:]) * lin.to(f0).view(1, -1, 1, 1) * (f0 / D - n1)
    u = torch.where(r > 0, f0 / torch.where(r > 0, r, torch.ones_like(r)), torch.zeros_like(f0))
    return (g - u * (u * g).sum(dim=1, keepdim=True) * (r / D)) / D


def lpips_gates(x, weights, normalize=False):
    """The ReLU masks and pool arg-max indices of the restatement's own forward on prepared images x [N,3,h,w]:
    ([mask per conv: bool [N,C,h,w]], [arg-max per pool: int64 [N,C,oh,ow], flat index into the pool's h*w input,
    first maximum in row-major window order])."""
    spec = _lpips_spec(weights['net'])
    if normalize:
        x = 2 * x - 1
    shift = torch.tensor(LPIPS_SHIFT, dtype=torch.float32).to(x).view(1, 3, 1, 1)
    scale = torch.tensor(LPIPS_SCALE, dtype=torch.float32).to(x).view(1, 3, 1, 1)
    x = (x - shift) / scale
    masks, argmax = [], []
    for op in spec['program']:
        if isinstance(op, int):
            _, _, _, s, p = spec['convs'][op]
            x = F.relu(F.conv2d(x, weights['conv_w'][op].to(x), weights['conv_b'][op].to(x), stride=s, padding=p))
            masks.append(x > 0)
        elif op != 'tap':
            x, idx = F.max_pool2d(x, op[1], op[2], return_indices=True)
            argmax.append(idx)
    return masks, argmax


def lpips_backward_reference(pred, gt, weights, masks=None, argmax=None, normalize=False, gvalue=None):
    """The gated backward of `lpips_value` on the host, in pred's dtype: (value [B], d(sum_b gvalue[b] value[b]) /
    d pred) for prepared (flipped, cropped) [B,3,h,w] images.  The forward is the restatement, but each ReLU passes
    where `masks` says so (one bool [B,C,h,w] per conv, for the pred images) and each max-pool takes the element
    `argmax` names (int64 [B,C,oh,ow] per pool, flat index into the pool's h*w input).  A pre-activation within
    rounding of zero, or two window elements within rounding of each other, may gate differently in another
    precision; with the gates of the run under test this is the gradient of the function that run computed.
    None: the forward's own gates, and the result is then autograd's gradient of `lpips_value`.  The gt half runs
    the plain restatement.  The per-layer distance takes the closed form `lpips_layer_grad` (finite at an all-zero
    pred vector)."""
    spec = _lpips_spec(weights['net'])
    B = pred.shape[0]
    if masks is None or argmax is None:
        own = lpips_gates(pred.detach(), weights, normalize)
        masks = own[0] if masks is None else masks
        argmax = own[1] if argmax is None else argmax
    with torch.no_grad():
        taps1 = lpips_features(gt.detach().to(pred.dtype), weights, normalize)
    x = pred.detach().clone().requires_grad_(True)
    leaf = x
    if normalize:
        x = 2 * x - 1
    shift = torch.tensor(LPIPS_SHIFT, dtype=torch.float32).to(x).view(1, 3, 1, 1)
    scale = torch.tensor(LPIPS_SCALE, dtype=torch.float32).to(x).view(1, 3, 1, 1)
    x = (x - shift) / scale
    taps0, ci, pi = [], 0, 0
    for op in spec['program']:
        if isinstance(op, int):
            _, _, _, s, p = spec['convs'][op]
            x = F.conv2d(x, weights['conv_w'][op].to(x), weights['conv_b'][op].to(x), stride=s, padding=p)
            x = x * masks[ci].to(x)
            ci += 1
        elif op == 'tap':
            taps0.append(x)
        else:
            idx = argmax[pi]
            x = x.flatten(2).gather(2, idx.flatten(2)).view(idx.shape)
            pi += 1
    gv = torch.ones(B, dtype=pred.dtype) if gvalue is None else gvalue.to(pred.dtype)
    value, grads = None, []
    for f0, f1, lin in zip(taps0, taps1, weights['lin']):
        f0d = f0.detach()
        m = lpips_layer_map(f0d, f1, lin).mean(dim=(1, 2))
        value = m if value is None else value + m
        hw = f0.shape[2] * f0.shape[3]
        grads.append(lpips_layer_grad(f0d, f1, lin, (gv / hw).view(B, 1, 1).expand(B, *f0.shape[2:])))
    torch.autograd.backward(taps0, grads)
    return value, leaf.grad


class _LPIPSDevice(torch.autograd.Function):
    """value [B] of ops.LPIPSPlan.forward with plan.backward as its gradient to pred."""

    @staticmethod
    def forward(ctx, pred, gt, plan, bi, bgr2rgb, normalize):
        value = plan.forward(pred.detach().float(), gt.detach().float().to(pred.device), bi, bgr2rgb, normalize)[0]
        ctx.plan, ctx.token, ctx.dtype = plan, plan.token(), pred.dtype
        return value.clone()

    @staticmethod
    def backward(ctx, gvalue):
        gpred = ctx.plan.backward(gvalue.float().contiguous(), token=ctx.token)
        return gpred.to(ctx.dtype, copy=True), None, None, None, None, None


class LPIPS(nn.Module):
    """models/loss/image_quality_v2.py:139-163 over lpips.LPIPS(net=type) (v0.1, spatial=False), restated: the
    optional channel flip [2,1,0], the boundary crop, the metric, the mean over the batch (`per_image`: [B]
    instead).  Images go in as they are, [0, 1], with the package's normalize=False as the reference calls it;
    `normalize=True` maps x -> 2x - 1 first.  `valid` is accepted and ignored, as in the reference.

    `weights` is anything `load_lpips_weights` takes (the package's state_dict, a torchvision backbone plus the
    head file as (backbone, heads), lists, or file paths); none are shipped or downloaded, and weights=None
    raises.  They are held as buffers, so .to(device) moves them.  Device tensors run the HIP plan
    (ops.LPIPSPlan: prep, fp32 convs, max-pools and the per-layer kernel); CPU tensors run the torch restatement
    `lpips_value`, which autograd differentiates.  Crops under 31 x 31 (alex) / 16 x 16 (vgg) raise ValueError.

    `differentiable=True` makes the device value a training objective: a device `pred` that requires grad goes
    through the plan's HIP backward (ops.LPIPSPlan.backward; the gradient reaches pred only -- gt.requires_grad
    raises ValueError; one forward per backward for a shape, a backward after a newer forward raises RuntimeError).
    At an all-zero feature vector of pred the gradient is the finite limit of the closed form, where the CPU path's
    autograd gives NaN.  By default the device path is forward-only and such a `pred` under enabled grad raises.
    CPU tensors ignore the flag."""

    def __init__(self, boundary_ignore=None, type='alex', bgr2rgb=False, weights=None, normalize=False,
                 per_image=False, differentiable=False):
        super().__init__()
        _lpips_spec(type)
        if weights is None:
            raise ValueError("LPIPS: weights=None. No pretrained weights are shipped or downloaded: pass the `lpips` "
                             "package's LPIPS(net=%r).state_dict() (or a file of it), a torchvision backbone "
                             "state_dict with the package's head file as (backbone, heads), or (conv_weights, "
                             "conv_biases, lins); generate_lpips_state_dict gives seeded stand-ins for tests" % type)
        if isinstance(weights, dict) and 'conv_w' in weights and weights.get('net') == type:
            w = weights
        elif isinstance(weights, (tuple, list)) and len(weights) == 2:
            w = load_lpips_weights(weights[0], type, heads=weights[1])
        else:
            w = load_lpips_weights(weights, type)
        self.boundary_ignore = boundary_ignore
        self.net = type
        self.bgr2rgb = bgr2rgb
        self.normalize = normalize
        self.per_image = per_image
        self.differentiable = bool(differentiable)
        self.n_convs = len(w['conv_w'])
        for i in range(self.n_convs):
            self.register_buffer('conv%d_weight' % i, w['conv_w'][i].clone())
            self.register_buffer('conv%d_bias' % i, w['conv_b'][i].clone())
        for l in range(5):
            self.register_buffer('lin%d' % l, w['lin'][l].clone())
        self._plan = None

    def weights(self):
        return {'net': self.net, 'conv_w': [getattr(self, 'conv%d_weight' % i) for i in range(self.n_convs)],
                'conv_b': [getattr(self, 'conv%d_bias' % i) for i in range(self.n_convs)],
                'lin': [getattr(self, 'lin%d' % l) for l in range(5)]}

    def plan(self):
        """The HIP plan for the buffers' device (rebuilt if the module moved)."""
        from . import ops
        if self._plan is None or self._plan.device != self.lin0.device:
            self._plan = ops.LPIPSPlan(self.weights())
        return self._plan

    def forward(self, pred, gt, valid=None):
        if pred.dim() == 3:
            pred, gt = pred.unsqueeze(0), gt.unsqueeze(0)
        bi = self.boundary_ignore or 0
        _lpips_check_crop(self.net, pred.shape[-2] - 2 * bi, pred.shape[-1] - 2 * bi)
        if pred.is_cuda:
            if self.differentiable and torch.is_grad_enabled() and gt.requires_grad:
                raise ValueError('LPIPS: gt.requires_grad on the device -- the HIP backward reaches pred only; detach gt')
            if self.differentiable and torch.is_grad_enabled() and pred.requires_grad:
                value = _LPIPSDevice.apply(pred, gt, self.plan(), bi, self.bgr2rgb, self.normalize)
                return value if self.per_image else value.mean()
            if torch.is_grad_enabled() and pred.requires_grad:
                raise RuntimeError('LPIPS: the device path is forward-only (no HIP backward): a gradient to pred would '
                                   'silently be zero.  Detach pred, score CPU tensors, or build the module with '
                                   'differentiable=True for the HIP backward')
            value = self.plan().forward(pred.detach().float(), gt.detach().float().to(pred.device), bi, self.bgr2rgb,
                                        self.normalize)[0].clone()
        else:
            p, g = lpips_prepare(pred, gt, self.boundary_ignore, self.bgr2rgb)
            value = lpips_value(p, g, self.weights(), self.normalize)[0]
        return value if self.per_image else value.mean()


# ------------------------------------------------------------------------------------------ harness

def _lpips_column(lpips, boundary_ignore, what):
    """The scorers' third column is an `LPIPS` module with the scorer's own crop."""
    if lpips is None:
        return None
    if (getattr(lpips, 'boundary_ignore', None) or 0) != (boundary_ignore or 0):
        raise ValueError('%s: lpips.boundary_ignore = %r, but the other columns are scored with %r'
                         % (what, getattr(lpips, 'boundary_ignore', None), boundary_ignore))
    return lpips


def _batches(dataset, batch, burst_sz):
    for s in range(0, len(dataset), batch):
        items = [dataset[i] for i in range(s, min(s + batch, len(dataset)))]
        bursts = torch.stack([it[0] for it in items])
        if burst_sz is not None:
            bursts = bursts[:, :burst_sz]
        yield bursts, torch.stack([it[1] for it in items]), [it[2]['burst_name'] for it in items]


def compute_score(net, dataset, boundary_ignore=40, burst_sz=None, device='cuda', batch=8, metrics=('psnr', 'ssim'),
                  lpips=None):
    """PSNR and SSIM columns of evaluation/synburst/compute_score.py:36-122 for one network: forward each
    burst, quantise like :109-111, per-image PSNR and SSIM with `boundary_ignore`, mean over the set.
    Bursts go through the engine `batch` at a time (bursts are independent); scores stay per image.
    Returns {'psnr': mean, 'per_image': {burst_name: psnr}, 'ssim': mean, 'per_image_ssim': {burst_name: ssim}}.

    `lpips` is an `LPIPS` module built with the caller's weights and this `boundary_ignore` (moved to `device` by
    the caller): the dict then gains 'lpips' (the mean) and 'per_image_lpips', the reference's third column,
    computed per image on the quantised prediction.  'lpips' in `metrics` is accepted only together with it; without
    a module it is an unknown metric, because there are no weights to compute it with.

    `metrics` may add 'msssim', the reference's MS-SSIM column: the dict then gains 'msssim' (the mean) and
    'per_image_msssim', computed per image on the quantised prediction with `boundary_ignore` like the other two.
    It is opt-in because MS-SSIM refuses crops under 32 x 32, which the other columns score, and because it is
    computed on the host (each quantised prediction is copied there; `MSSSIM` has no HIP kernel yet).  PSNR and
    SSIM are always reported."""
    unknown = set(metrics) - {'psnr', 'ssim', 'msssim'} - ({'lpips'} if lpips is not None else set())
    if unknown:
        raise ValueError('compute_score: unknown metrics %s' % sorted(unknown))
    psnr_fn = PSNR(boundary_ignore=boundary_ignore)
    ssim_fn = SSIM(boundary_ignore=boundary_ignore, use_for_loss=False)
    msssim_fn = MSSSIM(boundary_ignore=boundary_ignore, use_for_loss=False) if 'msssim' in metrics else None
    lpips_fn = _lpips_column(lpips, boundary_ignore, 'compute_score')
    per, per_ssim, per_ms, per_lp = {}, {}, {}, {}
    for bursts, gts, names in _batches(dataset, batch, burst_sz):
        with torch.no_grad():
            pred, _ = net(bursts.to(device))
        pred = quantize_prediction(pred.float())
        gts = gts.to(pred.device)
        for i, name in enumerate(names):
            per[name] = float(psnr_fn(pred[i:i + 1], gts[i:i + 1]))
            per_ssim[name] = float(ssim_fn(pred[i:i + 1], gts[i:i + 1]))
            if msssim_fn is not None:
                per_ms[name] = float(msssim_fn(pred[i:i + 1].cpu(), gts[i:i + 1].cpu()))   # host-side metric
            if lpips_fn is not None:
                with torch.no_grad():
                    per_lp[name] = float(lpips_fn(pred[i:i + 1], gts[i:i + 1]))
    res = {'psnr': sum(per.values()) / max(1, len(per)), 'per_image': per,
           'ssim': sum(per_ssim.values()) / max(1, len(per_ssim)), 'per_image_ssim': per_ssim}
    if msssim_fn is not None:
        res.update(msssim=sum(per_ms.values()) / max(1, len(per_ms)), per_image_msssim=per_ms)
    if lpips_fn is not None:
        res.update(lpips=sum(per_lp.values()) / max(1, len(per_lp)), per_image_lpips=per_lp)
    return res


def save_results(net, dataset, out_dir, burst_sz=None, device='cuda', batch=8):
    """evaluation/synburst/save_results.py:36-67: uint16 PNG of clamp(pred,0,1)*2^14 per burst, written
    the way cv2.imwrite writes an [H,W,3] array (array channels read as BGR)."""
    os.makedirs(out_dir, exist_ok=True)
    for bursts, _, names in _batches(dataset, batch, burst_sz):
        with torch.no_grad():
            pred, _ = net(bursts.to(device))
        arr = (pred.float().permute(0, 2, 3, 1).clamp(0.0, 1.0) * 2 ** 14).cpu().numpy().astype(np.uint16)
        for i, name in enumerate(names):
            imwrite('{}/{}.png'.format(out_dir, name), arr[i])


def load_saved_prediction(path):
    """compute_score.py:102-104: a saved prediction back to [1,3,H,W] float /2^14."""
    im = imread_unchanged(path)
    return (torch.from_numpy(im.astype(np.float32)) / 2 ** 14).permute(2, 0, 1).float().unsqueeze(0)


def save_visualization(net, dataset, out_dir, burst_sz=None, device='cuda', save_gt=False):
    """evaluation/synburst/visualize_results.py's image: each prediction turned into a viewable 8-bit sRGB PNG by
    synthetic.SimplePostProcess (the inverse camera pipeline, on the HIP kernel) and written with `png_write`
    (RGB order).  `dataset[i]` must be (burst [N,4,H,W], gt, meta_info) with the generator's meta_info keys
    (cam2rgb, rgb_gain, red_gain, blue_gain, gamma, smoothstep): SyntheticBurstVal, which does not unpickle its
    meta_info.pkl, is refused.  save_gt also writes <name>_gt.png.  Returns the written paths."""
    from .synthetic import SimplePostProcess
    post = SimplePostProcess(return_np=True)
    os.makedirs(out_dir, exist_ok=True)
    paths = []
    for i in range(len(dataset)):
        burst, gt, meta = dataset[i]
        missing = [k for k in ('cam2rgb', 'rgb_gain', 'red_gain', 'blue_gain', 'gamma', 'smoothstep') if k not in meta]
        if missing:
            raise ValueError('save_visualization: sample %d carries no camera meta_info (missing %s)' % (i, missing))
        if burst_sz is not None:
            burst = burst[:burst_sz]
        with torch.no_grad():
            pred, _ = net(burst.unsqueeze(0).to(device))
        name = meta.get('burst_name', '{:04d}'.format(i))
        path = os.path.join(out_dir, '{}.png'.format(name))
        png_write(path, post.process(pred[0].float(), meta))
        paths.append(path)
        if save_gt:
            png_write(os.path.join(out_dir, '{}_gt.png'.format(name)), post.process(gt.to(device).float(), meta))
    return paths
