"""What a depth-peeling layer costs: the forward time of `rasterize` and of layers 0-3 of a `DepthPeeler` on the bench's 70k noisy sphere
(tests/render_scenes.py: sphere70k) from B = 8 look-at views at 512 x 512. Layer 0 is rasterize's own native call; every later layer
walks all the triangles again and reads 8 bytes of the layer before per covering fragment, so about one rasterize each is the
expectation (a layer's figure also holds the copy the peeler keeps of it: 16 bytes per pixel). Each figure is the median over `repeats`
rounds of the time between two events around ONE call (idle gaps between the call's launches included), summed over `inner` passes and
divided by them; a round times rasterize and the four layers one after the other, so they alternate in one process. Nothing is
asserted. Writes one JSON document.
    python tools/bench_render_peel.py [out.json] [repeats]"""
import json
import os
import sys

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [_R, os.path.join(_R, "large-steps-pytorch_amd"), os.path.join(_R, "tests")]
import numpy as np
import torch
import largesteps.render as dr
from render_scenes import sphere70k

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(_R, "profiles", "render_peel_bench.json")
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 9
dev = torch.device("cuda:0")
B, RES, LAYERS, INNER = 8, 512, 4, 5

pos, tri, H, W = sphere70k(B, RES)
pos, tri = torch.from_numpy(pos).to(dev), torch.from_numpy(tri).to(dev)


def pair():
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def one_round():
    """ms per call: rasterize, then layers 0 .. LAYERS - 1, each between its own two events"""
    marks = {"rasterize": []}
    marks.update({f"layer{l}": [] for l in range(LAYERS)})
    torch.cuda.synchronize()
    for _ in range(INNER):
        a, b = pair()
        a.record()
        dr.rasterize(None, pos, tri, (H, W))
        b.record()
        marks["rasterize"].append((a, b))
        with dr.DepthPeeler(None, pos, tri, (H, W)) as peeler:
            for l in range(LAYERS):
                a, b = pair()
                a.record()
                peeler.rasterize_next_layer()
                b.record()
                marks[f"layer{l}"].append((a, b))
    torch.cuda.synchronize()
    return {k: sum(a.elapsed_time(b) for a, b in v) / INNER for k, v in marks.items()}


with torch.no_grad():
    with dr.DepthPeeler(None, pos, tri, (H, W)) as peeler:
        covered = [float((peeler.rasterize_next_layer()[0][..., 3] > 0).float().mean()) for _ in range(LAYERS)]
    for _ in range(2):
        one_round()
    rounds = [one_round() for _ in range(repeats)]

doc = {"device": torch.cuda.get_device_name(0), "mesh": "sphere70k", "V": int(pos.shape[1]), "F": int(tri.shape[0]), "B": B, "resolution": RES,
       "repeats": repeats, "inner": INNER, "unit": "ms (median over the rounds of the time between events around one forward call; a layer's call includes the peeler's copy of it)",
       "covered_fraction_per_layer": covered}
for k in rounds[0]:
    ts = [r[k] for r in rounds]
    doc[f"{k}_fwd_ms"] = float(np.median(ts))
    doc[f"{k}_fwd_min_max_ms"] = [float(min(ts)), float(max(ts))]
for l in range(LAYERS):
    doc[f"layer{l}_over_rasterize"] = doc[f"layer{l}_fwd_ms"] / doc["rasterize_fwd_ms"]
print(json.dumps(doc), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    json.dump(doc, fh, indent=1)
print("wrote", out_path)
