"""Synthetic training bursts on the device, and the way back to a viewable image.

The reference builds every training sample of its `default_synthetic` recipe with SyntheticBurstProcessing ->
rgb2rawburst (data/processing.py:38-123, data/synthetic_burst_generation.py:23-246, data/camera_pipeline.py): an sRGB
crop is unprocessed to linear sensor space, N randomly transformed and downsampled frames are made of it, and these
are mosaicked and corrupted by shot / read noise.  Here the random parameters are drawn on the host, consuming
Python's `random` and torch's CPU generator in the reference's order, and everything per pixel runs in the HIP
kernels of csrc/synth_ops.hip (ops.unprocess_rgb, ops.burst_synth): a batch of crops goes up once and the burst,
its ground truth and the flow stay on the device, ready for DBSRTrainer.step.

The warp is defined mathematically (include/dbsr_hip.h, DESIGN.md 'Synthetic training data'), in fp32 throughout.
The reference converts the unprocessed image to 8 bits and lets OpenCV warp and resize it in fixed point; that
difference is stated in DESIGN.md and has not been measured.

`process_linear_image_rgb` / `SimplePostProcess` (data/postprocessing_functions.py:19-50) invert the camera pipeline
with the `meta_info` the generator returns: ops.postprocess_rgb on device tensors, a torch restatement on CPU
tensors (the same split evaluation.SSIM uses).  The `*_cpu` functions restate the reference's arithmetic one image at
a time in the input's dtype; they are the oracle of the kernels and the CPU path, not a fall-back of the generator.
"""
import math
import random

import numpy as np
import torch

from . import ops

_IPP_DEFAULTS = {'random_ccm': True, 'random_gains': True, 'smoothstep': True, 'gamma': True, 'add_noise': True}

# XYZ -> camera matrices of four cameras and sRGB -> XYZ (Brooks et al., "Unprocessing Images for Learned Raw
# Denoising", CVPR 2019; camera_pipeline.py:30-53)
_XYZ2CAMS = [[[1.0234, -0.2969, -0.2266], [-0.5625, 1.6328, -0.0469], [-0.0703, 0.2188, 0.6406]],
             [[0.4913, -0.0541, -0.0202], [-0.613, 1.3513, 0.2906], [-0.1564, 0.2151, 0.7183]],
             [[0.838, -0.263, -0.0639], [-0.2887, 1.0725, 0.2496], [-0.0627, 0.1427, 0.5438]],
             [[0.6596, -0.2079, -0.0562], [-0.4782, 1.3016, 0.1933], [-0.097, 0.1581, 0.5181]]]
_RGB2XYZ = [[0.4124564, 0.3575761, 0.1804375], [0.2126729, 0.7151522, 0.0721750], [0.0193339, 0.1191920, 0.9503041]]


# ------------------------------------------------------------------------------------------ host samplers

def random_ccm():
    """camera_pipeline.random_ccm: a random convex combination of the four XYZ -> camera matrices (four uniforms
    from torch's CPU generator), times sRGB -> XYZ, each row normalised to sum 1.  float32 [3,3]."""
    xyz2cams = torch.tensor(_XYZ2CAMS)
    weights = torch.FloatTensor(len(_XYZ2CAMS), 1, 1).uniform_(0.0, 1.0)
    xyz2cam = (xyz2cams * weights).sum(dim=0) / weights.sum()
    rgb2cam = torch.mm(xyz2cam, torch.tensor(_RGB2XYZ))
    return rgb2cam / rgb2cam.sum(dim=-1, keepdim=True)


def random_gains():
    """camera_pipeline.random_gains: (rgb_gain, red_gain, blue_gain) = 1 / gauss(0.8, 0.1), uniform(1.9, 2.4),
    uniform(1.5, 1.9) from Python's `random`, in that order."""
    rgb_gain = 1.0 / random.gauss(mu=0.8, sigma=0.1)
    red_gain = random.uniform(1.9, 2.4)
    blue_gain = random.uniform(1.5, 1.9)
    return rgb_gain, red_gain, blue_gain


def random_noise_levels():
    """camera_pipeline.random_noise_levels: log-uniform shot noise in [1e-4, 0.012] and the read noise on the
    log-log line 2.18 x + 1.20 with gauss(0, 0.26) around it (Python's `random`: one uniform, one gauss)."""
    log_shot_noise = random.uniform(math.log(0.0001), math.log(0.012))
    shot_noise = math.exp(log_shot_noise)
    log_read_noise = 2.18 * log_shot_noise + 1.20 + random.gauss(mu=0.0, sigma=0.26)
    return shot_noise, math.exp(log_read_noise)


def sample_transform(params, downsample_factor, first=False):
    """One frame's transformation parameters (translation, theta, shear, scale) as single2lrburst:166-200 draws
    them.  The first frame is only shifted by f/2 - 0.5, to centre the sampling grid, and draws nothing.  Every
    other frame makes seven draws from Python's `random`, in this order: translation x, y, rotation, shear x, y,
    aspect ratio, scale -- each drawn even when its maximum is 0, except that, as in the reference,
    max_translation <= 0.01 takes the centring shift and skips the two translation draws."""
    params = params or {}
    shift = (downsample_factor / 2.0) - 0.5
    if first:
        return (shift, shift), 0.0, (0.0, 0.0), (1.0, 1.0)
    max_translation = params.get('max_translation', 0.0)
    if max_translation <= 0.01:
        translation = (shift, shift)
    else:
        translation = (random.uniform(-max_translation, max_translation),
                       random.uniform(-max_translation, max_translation))
    max_rotation = params.get('max_rotation', 0.0)
    theta = random.uniform(-max_rotation, max_rotation)
    max_shear = params.get('max_shear', 0.0)
    shear_x = random.uniform(-max_shear, max_shear)
    shear_y = random.uniform(-max_shear, max_shear)
    max_ar_factor = params.get('max_ar_factor', 0.0)
    ar_factor = np.exp(random.uniform(-max_ar_factor, max_ar_factor))
    max_scale = params.get('max_scale', 0.0)
    scale = np.exp(random.uniform(-max_scale, max_scale))
    return translation, theta, (shear_x, shear_y), (scale, scale * ar_factor)


def get_tmat(image_shape, translation, theta, shear_values, scale_factors):
    """synthetic_burst_generation.get_tmat in float64: the 2x3 matrix t_scale @ t_rot @ t_shear @ t_translate that
    maps a source pixel to its place in the transformed image.

    t_rot is cv2.getRotationMatrix2D((cx, cy), theta in degrees, 1.0) with (cx, cy) = (w / 2, h / 2), which the
    OpenCV documentation (imgproc, "Geometric Image Transformations") gives as
        [[ a,  b, (1 - a) cx - b cy],
         [-b,  a, b cx + (1 - a) cy]],   a = cos(theta), b = sin(theta)
    t_shear = [[1, sx, -sx w / 2], [sy, 1, -sy h / 2]], t_scale = diag(scale_x, scale_y)."""
    im_h, im_w = image_shape
    t_mat = np.identity(3)
    t_mat[0, 2] = translation[0]
    t_mat[1, 2] = translation[1]
    cx, cy = im_w * 0.5, im_h * 0.5
    a, b = math.cos(math.radians(theta)), math.sin(math.radians(theta))
    t_rot = np.array([[a, b, (1.0 - a) * cx - b * cy],
                      [-b, a, b * cx + (1.0 - a) * cy],
                      [0.0, 0.0, 1.0]])
    t_shear = np.array([[1.0, shear_values[0], -shear_values[0] * 0.5 * im_w],
                        [shear_values[1], 1.0, -shear_values[1] * 0.5 * im_h],
                        [0.0, 0.0, 1.0]])
    t_scale = np.array([[scale_factors[0], 0.0, 0.0],
                        [0.0, scale_factors[1], 0.0],
                        [0.0, 0.0, 1.0]])
    return (t_scale @ t_rot @ t_shear @ t_mat)[:2, :]


def inverse_tmat(t_mat):
    """The map from a pixel of the transformed image to its source position: the inverse of the 2x3 `t_mat` (what
    cv2.warpAffine applies per output pixel), float64 [2,3]."""
    m = np.concatenate([np.asarray(t_mat, dtype=np.float64), np.array([[0.0, 0.0, 1.0]])])
    return np.linalg.inv(m)[:2, :]


# ------------------------------------------------------------------------------------------ CPU restatements

def invert_smoothstep(image):
    image = image.clamp(0.0, 1.0)
    return 0.5 - torch.sin(torch.asin(1.0 - 2.0 * image) / 3.0)


def gamma_expansion(image):
    return image.clamp(1e-8) ** 2.2


def gamma_compression(image):
    return image.clamp(1e-8) ** (1.0 / 2.2)


def apply_smoothstep(image):
    return 3 * image ** 2 - 2 * image ** 3


def apply_ccm(image, ccm):
    shape = image.shape
    return torch.mm(ccm.to(image.device).type_as(image), image.reshape(3, -1)).view(shape)


def apply_gains(image, rgb_gain, red_gain, blue_gain):
    gains = (torch.tensor([red_gain, 1.0, blue_gain]) * rgb_gain).view(-1, 1, 1)
    return (image * gains.to(image.device).type_as(image)).clamp(0.0, 1.0)


def safe_invert_gains(image, rgb_gain, red_gain, blue_gain):
    gains = (torch.tensor([1.0 / red_gain, 1.0, 1.0 / blue_gain]) / rgb_gain).view(-1, 1, 1).to(image.device)
    gray = image.mean(dim=0, keepdim=True)
    inflection = 0.9
    mask = ((gray - inflection).clamp(0.0) / (1.0 - inflection)) ** 2.0
    return image * torch.max(mask + (1.0 - mask) * gains, gains)


def unprocess_rgb_cpu(image, rgb2cam, rgb_gain, red_gain, blue_gain, smoothstep=True, gamma=True):
    """rgb2rawburst:60-77 on one [3,H,W] image as torch ops in the image's dtype."""
    if smoothstep:
        image = invert_smoothstep(image)
    if gamma:
        image = gamma_expansion(image)
    image = apply_ccm(image, rgb2cam)
    image = safe_invert_gains(image, rgb_gain, red_gain, blue_gain)
    return image.clamp(0.0, 1.0)


def mosaic(image):
    """camera_pipeline.mosaic, 'rggb': [..., 3, H, W] -> [..., 4, H/2, W/2] planes R, Gr, Gb, B."""
    return torch.stack((image[..., 0, 0::2, 0::2], image[..., 1, 0::2, 1::2], image[..., 1, 1::2, 0::2],
                        image[..., 2, 1::2, 1::2]), dim=-3)


def add_noise_cpu(image, shot_noise, read_noise, z):
    """camera_pipeline.add_noise with the standard normals `z` given (the reference draws them from torch's CPU
    generator), then rgb2rawburst's clamp."""
    variance = image * shot_noise + read_noise
    return (image + z.to(image.device) * variance.sqrt()).clamp(0.0, 1.0)


def process_linear_image_rgb_cpu(image, meta_info, gains=True, ccm=True, gamma=True, smoothstep=True):
    """postprocessing_functions.process_linear_image_rgb on one [3,H,W] image as torch ops in its dtype."""
    if gains:
        image = apply_gains(image, meta_info['rgb_gain'], meta_info['red_gain'], meta_info['blue_gain'])
    if ccm:
        image = apply_ccm(image, meta_info['cam2rgb'])
    image = image.clamp(0.0, 1.0)
    if meta_info['gamma'] and gamma:
        image = gamma_compression(image)
    if meta_info['smoothstep'] and smoothstep:
        image = apply_smoothstep(image)
    return image.clamp(0.0, 1.0)


# ------------------------------------------------------------------------------------------ the generator

def _pack_params(mats, rgb, red, blue, smoothstep, gamma):
    """[B,16] float32 rows of dbsr_hip.h's `params`: 9 matrix entries, rgb / red / blue gain, two flags, 2 spare."""
    B = len(rgb)
    p = torch.zeros(B, 16, dtype=torch.float32)
    p[:, :9] = torch.stack([m.reshape(9).float() for m in mats])
    p[:, 9] = torch.tensor(rgb, dtype=torch.float64).float()
    p[:, 10] = torch.tensor(red, dtype=torch.float64).float()
    p[:, 11] = torch.tensor(blue, dtype=torch.float64).float()
    p[:, 12] = torch.tensor([1.0 if s else 0.0 for s in smoothstep])
    p[:, 13] = torch.tensor([1.0 if g else 0.0 for g in gamma])
    return p


def _image_processing_params(image_processing_params):
    ipp = dict(_IPP_DEFAULTS)
    ipp.update(image_processing_params or {})
    return ipp


def sample_camera(image_processing_params):
    """The draws rgb2rawburst:47-58 makes before it touches the image: (rgb2cam, rgb_gain, red_gain, blue_gain)."""
    rgb2cam = random_ccm() if image_processing_params['random_ccm'] else torch.eye(3).float()
    gains = random_gains() if image_processing_params['random_gains'] else (1.0, 1.0, 1.0)
    return (rgb2cam,) + tuple(gains)


def _sample_one(shape, burst_size, f, btp, ipp):
    """One image's random parameters, drawn in rgb2rawburst's order: camera, the burst's transforms, noise levels."""
    rgb2cam, rgb_gain, red_gain, blue_gain = sample_camera(ipp)
    ainv = np.stack([inverse_tmat(get_tmat(shape, *sample_transform(btp, f, first=(n == 0)))) for n in range(burst_size)])
    shot, read = random_noise_levels() if ipp['add_noise'] else (0, 0)
    return {'rgb2cam': rgb2cam, 'cam2rgb': rgb2cam.inverse(), 'rgb_gain': rgb_gain, 'red_gain': red_gain,
            'blue_gain': blue_gain, 'ainv': ainv, 'shot_noise_level': shot, 'read_noise_level': read}


def _generate(images, samples, downsample_factor, border_crop, ipp, generator, want_rgb=True, want_flow=True):
    """The device part of rgb2rawburst for a batch whose per-image parameters `samples` are drawn."""
    dev = images.device
    B = images.shape[0]
    params = _pack_params([s['rgb2cam'] for s in samples], [s['rgb_gain'] for s in samples],
                          [s['red_gain'] for s in samples], [s['blue_gain'] for s in samples],
                          [ipp['smoothstep']] * B, [ipp['gamma']] * B).to(dev)
    lin = ops.unprocess_rgb(images, params)
    ainv = torch.from_numpy(np.stack([s['ainv'] for s in samples])).float().to(dev)
    N = ainv.shape[1]
    Hc, Wc = lin.shape[-2:]
    bc, f = int(border_crop or 0), int(downsample_factor)
    levels = z = None
    if ipp['add_noise']:
        levels = torch.tensor([[s['shot_noise_level'], s['read_noise_level']] for s in samples],
                              dtype=torch.float64).float().to(dev)
        z = torch.randn(B, N, 4, (Hc - 2 * bc) // f // 2, (Wc - 2 * bc) // f // 2, device=dev, generator=generator)
    burst, burst_rgb, flow = ops.burst_synth(lin, ainv, bc, f, levels, z, want_rgb=want_rgb, want_flow=want_flow)
    return burst, lin, burst_rgb, flow


def _meta(samples, ipp, single):
    if single:
        s = samples[0]
        m = {k: s[k] for k in ('rgb2cam', 'cam2rgb', 'rgb_gain', 'red_gain', 'blue_gain')}
        m.update(smoothstep=ipp['smoothstep'], gamma=ipp['gamma'], shot_noise_level=s['shot_noise_level'],
                 read_noise_level=s['read_noise_level'])
        return m
    m = {k: torch.stack([s[k] for s in samples]) for k in ('rgb2cam', 'cam2rgb')}
    for k in ('rgb_gain', 'red_gain', 'blue_gain', 'shot_noise_level', 'read_noise_level'):
        m[k] = torch.tensor([s[k] for s in samples], dtype=torch.float64)
    m.update(smoothstep=ipp['smoothstep'], gamma=ipp['gamma'])
    return m


def _as_batch(images):
    """([B,3,H,W] float32 or [B,H,W,3] uint8, single?) of a device image or batch in either layout."""
    if not torch.is_tensor(images):
        raise TypeError('images must be a torch tensor on the HIP device')
    single = images.dim() == 3
    if single:
        images = images.unsqueeze(0)
    if images.dim() != 4:
        raise ValueError('images must be [B,3,H,W] / [3,H,W] float or [B,H,W,3] / [H,W,3] uint8')
    if images.dtype == torch.uint8:
        if images.shape[-1] != 3:
            raise ValueError('uint8 images must be [.., H, W, 3] RGB')
    else:
        if images.shape[1] != 3:
            raise ValueError('float images must be [.., 3, H, W]')
        images = images.float()
    return images, single


def _check_interpolation(interpolation_type):
    if interpolation_type == 'lanczos':
        raise NotImplementedError("interpolation_type='lanczos' is not implemented (bilinear only)")
    if interpolation_type != 'bilinear':
        raise ValueError('interpolation_type %r' % (interpolation_type,))


def rgb2rawburst(images, burst_size, downsample_factor=1, burst_transformation_params=None,
                 image_processing_params=None, interpolation_type='bilinear', generator=None):
    """synthetic_burst_generation.rgb2rawburst on the device.  images: [B,3,Hc,Wc] float in [0,1] or [B,Hc,Wc,3]
    uint8 (a single image gives outputs without the batch dimension).  Returns the reference's tuple
    (burst [B,N,4,H2/2,W2/2], frame_gt_full [B,3,Hc,Wc] linear, burst_rgb [B,N,3,H2,W2], flow_vectors [B,N,2,H2,W2],
    meta_info).  The host draws follow the reference's order per image (Python `random`, torch's CPU generator);
    the noise normals come from torch.randn on the device with `generator`."""
    _check_interpolation(interpolation_type)
    images, single = _as_batch(images)
    ops._need_cuda(images)
    ipp = _image_processing_params(image_processing_params)
    btp = burst_transformation_params or {}
    shape = tuple(images.shape[1:3]) if images.dtype == torch.uint8 else tuple(images.shape[2:4])
    samples = [_sample_one(shape, burst_size, downsample_factor, btp, ipp) for _ in range(images.shape[0])]
    burst, lin, burst_rgb, flow = _generate(images, samples, downsample_factor, btp.get('border_crop'), ipp, generator)
    out = (burst, lin, burst_rgb, flow)
    if single:
        out = tuple(t[0] for t in out)
    return out + (_meta(samples, ipp, single),)


class SyntheticBurstProcessing:
    """data/processing.py:38-123 for a batch: a padded random (or centre) crop of each image by slicing on the
    host, one upload, rgb2rawburst on the device.  __call__ takes a list of [H,W,3] uint8 images (numpy or torch)
    or a uint8 batch [B,H,W,3], and returns {'burst', 'frame_gt' (border-cropped), 'meta_info'[, 'burst_rgb']} on
    `device`: DBSRTrainer.step(d['burst'], d['frame_gt'])."""

    def __init__(self, crop_sz, burst_size, downsample_factor, crop_scale_range=None, crop_ar_range=None,
                 burst_transformation_params=None, image_processing_params=None, interpolation_type='bilinear',
                 return_rgb_busrt=False, random_crop=True, device='cuda', generator=None):
        if crop_scale_range is not None or crop_ar_range is not None:
            raise NotImplementedError('crop_scale_range / crop_ar_range: random resized crops are not implemented')
        _check_interpolation(interpolation_type)
        self.crop_sz = tuple(crop_sz) if isinstance(crop_sz, (tuple, list)) else (crop_sz, crop_sz)
        self.burst_size = burst_size
        self.downsample_factor = downsample_factor
        self.burst_transformation_params = burst_transformation_params or {}
        self.image_processing_params = image_processing_params
        self.return_rgb_busrt = return_rgb_busrt
        self.random_crop = random_crop
        self.device = device
        self.generator = generator

    def _crop(self, img, crop_sz):
        img = torch.as_tensor(img)
        if img.dim() != 3 or img.shape[-1] != 3 or img.dtype != torch.uint8:
            raise ValueError('SyntheticBurstProcessing: images must be [H,W,3] uint8')
        H, W = img.shape[:2]
        if H < crop_sz[0] or W < crop_sz[1]:
            raise NotImplementedError('image %dx%d is smaller than the padded crop %dx%d (the reference resizes it)'
                                      % (H, W, crop_sz[0], crop_sz[1]))
        if self.random_crop:          # processing_utils.random_resized_crop without scale / aspect ranges
            r1 = random.randint(0, H - crop_sz[0])
            c1 = random.randint(0, W - crop_sz[1])
        else:                         # processing_utils.center_crop
            r1, c1 = (H - crop_sz[0]) // 2, (W - crop_sz[1]) // 2
        return img[r1:r1 + crop_sz[0], c1:c1 + crop_sz[1]]

    def __call__(self, images):
        btp = self.burst_transformation_params
        bc = btp.get('border_crop')
        crop_sz = [c + 2 * btp.get('border_crop', 0) for c in self.crop_sz]
        ipp = _image_processing_params(self.image_processing_params)
        crops, samples = [], []
        for img in images:            # per image: the crop's draws, then rgb2rawburst's, as one reference sample
            crops.append(self._crop(img, crop_sz))
            samples.append(_sample_one(tuple(crop_sz), self.burst_size, self.downsample_factor, btp, ipp))
        batch = torch.stack(crops).contiguous().to(self.device)
        burst, lin, burst_rgb, _ = _generate(batch, samples, self.downsample_factor, bc, ipp, self.generator,
                                             want_rgb=self.return_rgb_busrt, want_flow=False)
        frame_gt = lin[..., bc:-bc, bc:-bc].contiguous() if bc else lin
        data = {'burst': burst, 'frame_gt': frame_gt, 'meta_info': _meta(samples, ipp, False)}
        if self.return_rgb_busrt:
            data['burst_rgb'] = burst_rgb
        return data


# ------------------------------------------------------------------------------------------ postprocess

def _meta_item(meta_info, b, B):
    """Image b's meta_info out of a batched one (tensors [B, ...]) or a single one shared by the batch."""
    out = {}
    for k in ('cam2rgb', 'rgb_gain', 'red_gain', 'blue_gain', 'gamma', 'smoothstep'):
        v = meta_info[k]
        if torch.is_tensor(v):
            if k == 'cam2rgb':
                v = v[b] if v.dim() == 3 else v
            else:
                v = v.reshape(-1)
                v = v[b if v.numel() == B and B > 1 else 0].item()
        elif isinstance(v, (list, tuple)):
            v = v[b]
        out[k] = v
    return out


def process_linear_image_rgb(image, meta_info, gains=True, ccm=True, gamma=True, smoothstep=True, return_np=False):
    """postprocessing_functions.process_linear_image_rgb: linear sensor image [3,H,W] or [B,3,H,W] -> sRGB in [0,1]
    with the generator's `meta_info` (batched or single).  Device tensors run ops.postprocess_rgb, CPU tensors the
    torch restatement.  return_np: the uint8 [H,W,3] / [B,H,W,3] RGB array, (uint8)(v * 255) truncated as
    torch_to_npimage does (RGB order: evaluation.png_write takes RGB; the reference swaps to BGR for cv2.imwrite)."""
    single = image.dim() == 3
    img = image.unsqueeze(0) if single else image
    B = img.shape[0]
    metas = [_meta_item(meta_info, b, B) for b in range(B)]
    if img.is_cuda:
        params = _pack_params([m['cam2rgb'] for m in metas], [m['rgb_gain'] for m in metas],
                              [m['red_gain'] for m in metas], [m['blue_gain'] for m in metas],
                              [m['smoothstep'] for m in metas], [m['gamma'] for m in metas]).to(img.device)
        out, u8 = ops.postprocess_rgb(img.float(), params, gains, ccm, gamma, smoothstep, want_f32=not return_np,
                                      want_u8=return_np)
        if return_np:
            out = u8.cpu().numpy()
    else:
        out = torch.stack([process_linear_image_rgb_cpu(img[b], metas[b], gains, ccm, gamma, smoothstep)
                           for b in range(B)])
        if return_np:
            out = (out.permute(0, 2, 3, 1).float().numpy() * 255).astype(np.uint8)
    return out[0] if single else out


class SimplePostProcess:
    """postprocessing_functions.SimplePostProcess."""

    def __init__(self, gains=True, ccm=True, gamma=True, smoothstep=True, return_np=False):
        self.gains, self.ccm, self.gamma, self.smoothstep, self.return_np = gains, ccm, gamma, smoothstep, return_np

    def process(self, image, meta_info):
        return process_linear_image_rgb(image, meta_info, self.gains, self.ccm, self.gamma, self.smoothstep,
                                        self.return_np)
