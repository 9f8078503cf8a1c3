"""Pins of the oracle to the reference model, on stored vectors (tests/golden/pin_128.*, written by tests/golden/make_golden.py from
the reference's own code): the weight spec against the reference's state_dict, and the oracle against the reference's forward."""
import json
import os

import torch

from golden_utils import GOLDEN, compare_summary, load_npz


def test_weight_spec_and_forward_match_reference():
    from oracle import siu3r_oracle as O
    from oracle import weights as OW

    z = load_npz("pin_128")
    meta = json.load(open(os.path.join(GOLDEN, "pin_128.json")))
    sd = OW.make_weights(0)
    ref_spec = {k: (tuple(shape), dtype) for k, shape, dtype in meta["state_dict"]}
    assert set(ref_spec) == set(sd)
    assert all(ref_spec[k] == (tuple(sd[k].shape), str(sd[k].dtype)) for k in ref_spec)
    g = torch.Generator().manual_seed(0)
    img = torch.rand(1, 2, 3, 128, 128, generator=g)
    K = torch.tensor([[318 / 256, 0, 0.5], [0, 318 / 256, 0.5], [0, 0, 1]])[None, None].repeat(1, 2, 1, 1)
    with torch.no_grad():
        out = O.model_forward(sd, img, K, keep_intermediates=False)
    for f in ("means", "covariances", "opacities", "scales", "rotations"):
        a, b = out[f], torch.from_numpy(z[f])
        assert a.shape == b.shape, (f, a.shape, b.shape)
        assert float((a - b).abs().max()) <= 5e-5 * float(b.abs().max()), f
    compare_summary("harmonics", out["harmonics"], z, 5e-5)  # (9.8 MB whole: strided samples + a dense window + the norm)
    # the logits are bit-identical to the reference's at the thread count the vectors were recorded with; fp32 CPU sums reorder with
    # the thread partition (1 / 3 threads: <= 2e-6 max-normalised), so the stored form bounds them at 1e-5
    for f in ("class_queries_logits", "masks_queries_logits"):
        a, b = out[f], torch.from_numpy(z[f])
        assert a.shape == b.shape, (f, a.shape, b.shape)
        assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max()), f
    strip = lambda segs: [[(s_["id"], s_["label_id"], s_["was_fused"]) for s_ in i] for i in segs]
    assert strip(out["seg_infos"]) == strip(meta["seg_infos"]) and len(meta["seg_infos"][0]) >= 3
