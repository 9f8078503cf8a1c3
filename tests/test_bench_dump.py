"""bench.py --dump-outputs on the host: the writer's budget, dtypes and seeded samples (stand-in outputs; the GPU run is in
tests/test_bench_gpu.py)."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from siu3r_amd.gaussians_types import Gaussians  # noqa: E402


def _outputs(N, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    gs = Gaussians(r(1, N, 3), r(1, N, 3, 3), r(1, N, 3, 25), torch.rand(1, N, generator=g), r(1, N, 3), r(1, N, 4))
    gs.semantic_labels = torch.randint(0, 21, (1, N), generator=g)
    gs.instance_labels = torch.randint(0, 9, (1, N), generator=g)
    gs.seg_query_class_logits = [r(N, 3, 21)]
    seg = {"loss": None, "class_queries_logits": r(1, 100, 21), "masks_queries_logits": r(1, 100, 2, 16, 16).bfloat16(), "_private": r(4)}
    masks = [torch.randint(-1, 4, (2, 16, 16), dtype=torch.int32, generator=g)]
    infos = [[{"id": 1, "label_id": 3, "was_fused": False, "score": 0.93}, {"id": 2, "label_id": 0, "was_fused": True, "score": 0.81}]]
    return gs, seg, masks, infos, [[0.93, 0.81, 0.4]]


def test_dump_outputs_budget_dtypes_and_samples(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 2 << 20)  # small budget: the large arrays are sampled
    out = _outputs(2 * 16 * 16 * 32, 0)
    a_dir, b_dir = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(out, str(a_dir))
    bench.dump_outputs(out, str(b_dir))
    m = json.load(open(a_dir / "manifest.json"))
    assert "seg__private" not in m["arrays"] and "seg_loss" not in m["arrays"]
    total = 0
    for n, e in m["arrays"].items():
        a, b = np.load(a_dir / f"{n}.npy"), np.load(b_dir / f"{n}.npy")
        assert np.array_equal(a, b), n  # same outputs -> the same files
        assert a.dtype == (np.float64 if n.startswith(("segments", "query_scores", "seg_masks_0")) or "labels" in n else np.float32), (n, a.dtype)
        assert list(a.shape) == ([e["sample"]["elements"]] if "sample" in e else e["shape"]), n
        total += a.nbytes
    assert total <= bench.DUMP_BYTES and "sample" in m["arrays"]["gaussians_harmonics"]
    assert np.array_equal(np.load(a_dir / "segments_0.npy"), [[1, 3, 0, 0.93], [2, 0, 1, 0.81]])
    assert np.array_equal(np.load(a_dir / "seg_masks_0.npy"), out[2][0].double().numpy())
    assert np.array_equal(np.load(a_dir / "seg_masks_queries_logits.npy"), out[1]["masks_queries_logits"].float().numpy())
