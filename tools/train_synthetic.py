"""A minimal training loop on synthetic bursts made from a folder of PNG images, with the settings of the reference's
train_settings/dbsr/default_synthetic.py as defaults: crops of 384, bursts of 8, downsample factor 4, translations up
to 24 px, rotations up to 1 degree, a border of 24 px.

Every step reads `--batch` random images with evaluation.png_read, lets synthetic.SyntheticBurstProcessing crop them on
the host and make the RAW bursts and the linear ground truth on the GPU, and gives both to DBSRTrainer.step.  Images
smaller than crop + 2 * border (432 px) are skipped when the folder is listed.  The network starts from the seeded
synthetic weights unless --weights names a state dict.

--dtype picks the compute dtype (bf16 default; fp16 trains with DBSRTrainer's dynamic loss scaler, whose state is
printed with the loss; fp32).

The loss is DBSRTrainer's objective (dbsr_amd.objectives.Objective), so every choice below keeps the fused step --
graph replay, the bucketed all-reduce, fused Adam, the device-side loss scaler:
--metric l1|l2|l2_sqrt|charbonnier picks the pixel-wise term (PixelWiseError, boundary_ignore 40);
--ssim W adds W * (1 - SSIM) with a dynamic range of 1, inside the plan;
--lpips FILE adds --lpips-weight * LPIPS(pred, gt): FILE is anything evaluation.load_lpips_weights reads (the `lpips`
package's LPIPS(net).state_dict() saved with torch.save; none are shipped).  The metric's HIP forward and backward
(evaluation.LPIPS(differentiable=True)) run eagerly between the plan's forward and backward.
The printed line is trainer.last_stats (Loss/total, Loss/rgb, Stat/psnr, ...), read back only where it is printed.

Usage: python tools/train_synthetic.py IMAGE_DIR [--steps 100 --batch 16 --lr 1e-4 --seed 0 --dtype bf16 --save out.pth
           --metric l1 --ssim W --lpips FILE --lpips-weight 0.1 --lpips-net alex|vgg]"""
import argparse
import os
import random
import struct
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dbsr_amd  # noqa: E402
from dbsr_amd.evaluation import png_read  # noqa: E402
from dbsr_amd.synthetic import SyntheticBurstProcessing  # noqa: E402
from dbsr_amd.training import DBSRTrainer  # noqa: E402


def png_size(path):
    with open(path, 'rb') as f:
        head = f.read(24)
    return struct.unpack('>II', head[16:24]) if head[12:16] == b'IHDR' else (0, 0)


def load_rgb8(path):
    img = png_read(path)
    if img.dtype != 'uint8':
        img = (img >> 8).astype('uint8')
    if img.shape[2] == 1:
        img = img.repeat(3, axis=2)
    return img[:, :, :3]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('image_dir')
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--crop', type=int, default=384)
    ap.add_argument('--burst', type=int, default=8)
    ap.add_argument('--factor', type=int, default=4)
    ap.add_argument('--max-translation', type=float, default=24.0)
    ap.add_argument('--max-rotation', type=float, default=1.0)
    ap.add_argument('--border-crop', type=int, default=24)
    ap.add_argument('--lr', type=float, default=1e-4)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--dtype', choices=['bf16', 'fp16', 'fp32'], default='bf16')
    ap.add_argument('--weights', default=None)
    ap.add_argument('--save', default=None)
    ap.add_argument('--metric', choices=['l1', 'l2', 'l2_sqrt', 'charbonnier'], default='l1')
    ap.add_argument('--ssim', type=float, default=None, help='weight of the (1 - SSIM) term')
    ap.add_argument('--lpips', default=None, help='LPIPS weights file: adds --lpips-weight * LPIPS(pred, gt) to the loss')
    ap.add_argument('--lpips-weight', type=float, default=0.1)
    ap.add_argument('--lpips-net', choices=['alex', 'vgg'], default='alex')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('train_synthetic: no HIP device')
    random.seed(args.seed)
    torch.manual_seed(args.seed)
    dev = torch.device('cuda')
    need = args.crop + 2 * args.border_crop
    files = sorted(os.path.join(args.image_dir, n) for n in os.listdir(args.image_dir) if n.lower().endswith('.png'))
    files = [p for p in files if min(png_size(p)) >= need]
    if not files:
        sys.exit('train_synthetic: no PNG of at least %d x %d pixels in %s' % (need, need, args.image_dir))

    net = dbsr_amd.build_synthetic_net(seed=0)
    if args.weights:
        net.load_state_dict(torch.load(args.weights, map_location='cpu'))
    dtype = {'bf16': torch.bfloat16, 'fp16': torch.float16, 'fp32': torch.float32}[args.dtype]
    net = net.to(dev).set_compute_dtype(dtype)
    objective = None                      # the built-in L1 plan
    if args.metric != 'l1' or args.ssim is not None or args.lpips:
        from dbsr_amd.objectives import Objective
        extra = None
        if args.lpips:
            from dbsr_amd.evaluation import LPIPS
            lpips = LPIPS(boundary_ignore=40, type=args.lpips_net, weights=args.lpips, differentiable=True).to(dev)
            extra = lambda pred, gt: args.lpips_weight * lpips(pred, gt)          # noqa: E731
        objective = Objective(args.metric, ssim=args.ssim, extra=extra, boundary_ignore=40)
    trainer = DBSRTrainer(net, lr=args.lr, objective=objective)
    btp = {'max_translation': args.max_translation, 'max_rotation': args.max_rotation, 'max_shear': 0.0,
           'max_scale': 0.0, 'border_crop': args.border_crop}
    proc = SyntheticBurstProcessing(args.crop, args.burst, args.factor, burst_transformation_params=btp,
                                    image_processing_params={'random_ccm': True, 'random_gains': True,
                                                             'smoothstep': True, 'gamma': True, 'add_noise': True},
                                    device=dev, generator=torch.Generator(device=dev).manual_seed(args.seed))
    for step in range(args.steps):
        d = proc([load_rgb8(random.choice(files)) for _ in range(args.batch)])
        loss = trainer.step(d['burst'], d['frame_gt'])
        if step % 10 == 0 or step == args.steps - 1:
            ls = trainer.loss_scale_state()          # (a small device-to-host copy: only where the loss is printed)
            scaler = '' if ls is None else '  scale %g  applied %d  skipped %d' % (ls['scale'], ls['steps'], ls['skipped'])
            stats = trainer.last_stats or {}
            terms = ''.join('  %s %.5f' % (k, float(v)) for k, v in stats.items() if k != 'Loss/total')
            print('step %d  loss %.5f%s%s' % (step, float(loss), terms, scaler), flush=True)
    if args.save:
        torch.save(net.state_dict(), args.save)


if __name__ == '__main__':
    main()
