"""Golden fixtures for the WeightedSum constructor variants (merging.py:23-32, 79-121), made by running the REFERENCE.

Build container only (needs /root/reference; the GPU box never runs this).  Same import recipe as make_golden.py
(cupy / lpips / admin.local stubs, the oracle's correlation for the reference's CUDA-only FunctionCorrelation, PWC-Net
with load_pretrained=False, weights from dbsr_amd.weights.generate_state_dict(seed=0)).  Writes
tests/golden/variants.part*.npz:
  merging_<case>_*   the reference WeightedSum module alone on random embeddings and offsets reaching well past
                     [-1, 1) (so offset_modulo matters), small dims
  e2e_<case>_*       the reference dbsrnet_cvpr2021 at the synthetic architecture, B=1 N=4 48x48, variant flags set
Cases: softmax=False ('relu'), use_base_frame=False ('mean'), offset_modulo=None ('nomod'), all three ('all').

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_variants.py
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = '/root/reference'

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, HERE)
from make_golden import _install_stubs  # noqa: E402

CASES = {
    'relu': dict(softmax=False),
    'mean': dict(use_base_frame=False),
    'nomod': dict(offset_modulo=None),
    'all': dict(softmax=False, use_base_frame=False, offset_modulo=None),
}
MERGING_DIMS = dict(input_dim=32, project_dim=32, offset_feat_dim=16)


def main():
    sys.path.insert(0, REPO)
    from oracle import dbsr_oracle as orc
    import dbsr_amd
    from dbsr_amd import arch
    from dbsr_amd.weights import generate_state_dict
    from dbsr_amd.burst import synthetic_bursts

    _install_stubs()
    sys.path.insert(0, REF)
    import models.alignment.pwcnet as ref_pwc
    import models.dbsr.dbsrnet as ref_dbsrnet
    import models.dbsr.merging as ref_merging

    ref_pwc.correlation.FunctionCorrelation = lambda tenFirst, tenSecond: orc.correlation(tenFirst, tenSecond)
    ref_dbsrnet.PWCNet = lambda load_pretrained=True, weights_path=None: ref_pwc.PWCNet(load_pretrained=False)
    torch.manual_seed(0)
    torch.set_num_threads(os.cpu_count())
    out = {}

    # ---------------- WeightedSum alone ----------------
    g = torch.Generator().manual_seed(77)
    B, N, C, H, W = 2, 4, MERGING_DIMS['input_dim'], 8, 10
    ref_feat = torch.rand(B, N - 1, C, H, W, generator=g)       # ReLU embeddings (>= 0), reference frame repeated
    ref_feat[:, 1:] = ref_feat[:, :1]
    oth_feat = torch.rand(B, N - 1, C, H, W, generator=g)
    offsets = (torch.rand(B, N - 1, 2, H, W, generator=g) - 0.5) * 6.0
    out['merging_ref_feat'], out['merging_oth_feat'] = ref_feat.numpy(), oth_feat.numpy()
    out['merging_offsets'] = offsets.numpy()
    for case, flags in CASES.items():
        m = ref_merging.WeightedSum(**MERGING_DIMS, **dict(dict(offset_modulo=1.0, use_base_frame=True), **flags))
        shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
        sd = generate_state_dict(shapes, seed=5)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        with torch.no_grad():
            r = m.eval()({'ref_feat': ref_feat, 'oth_feat': oth_feat, 'offsets': offsets})
        out[f'merging_{case}_fused'] = r['fused_enc'].numpy()
        out[f'merging_{case}_weights'] = r['fusion_weights'].numpy()
        if case == 'relu':
            for k, v in sd.items():
                out['merging_sd.' + k] = v
        print('merging', case, float(r['fused_enc'].mean()), float(r['fusion_weights'].std()))

    # ---------------- whole network ----------------
    kw0 = dict(orc.DBSR_SYNTHETIC_KWARGS)
    burst, _ = synthetic_bursts(1, 4, 48, 48, sr_factor=8, seed=21)
    out['e2e_burst'] = burst.numpy()
    for case, flags in CASES.items():
        kw = dict(kw0, **flags)
        ref_net = ref_dbsrnet.dbsrnet_cvpr2021(**kw).eval()
        shapes = arch.state_dict_shapes(dbsr_amd.dbsrnet_cvpr2021(**kw))
        assert shapes == arch.state_dict_shapes(ref_net), 'state_dict mismatch'
        sd = generate_state_dict(shapes, seed=0)
        ref_net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        with torch.no_grad():
            pred, aux = ref_net(burst)
        fw = aux['fusion_weights']
        out[f'e2e_{case}_pred_crop'] = pred[..., 100:164, 100:164].numpy()
        out[f'e2e_{case}_pred_sum'] = pred.double().sum(dim=(-2, -1)).float().numpy()
        out[f'e2e_{case}_fw_sum'] = fw.double().sum(dim=(-2, -1)).float().numpy()
        out[f'e2e_{case}_fw_crop'] = fw[:, :, :16, 8:16, 8:16].numpy()
        if case == 'relu':
            out['e2e_offsets'] = aux['offsets'].numpy()
        print('e2e', case, 'pred mean', float(pred.mean()), 'offs absmax', float(aux['offsets'].abs().max()))

    import npz_parts
    for path in npz_parts.save(HERE, 'variants', out):
        print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
