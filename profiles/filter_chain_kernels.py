"""Which filter kernels the chain launches, per case — the recipe of profiles/filter_chain_kernels.txt.

    rocprofv3 --kernel-trace --output-format csv -d OUT -o chain -- python3 profiles/filter_chain_kernels.py run OUT/labels.txt
    python3 profiles/filter_chain_kernels.py list OUT/chain_kernel_trace.csv OUT/labels.txt

run:  one whole-map chain (fpe_traversability_device, no layer buffer) and one fpe_update_elevation with the single patch
      (30, 14, 4, 4) per case of tests/test_cpu_filter_route.py (TABLE, then FALLBACKS), each behind a marker kernel (a torch fill);
      the steps' labels, in order, go to the file named.
run-forms: the same two steps per case of tests/filter_form_cases.py (one case per kernel form, shift (5, 3), the case's own map
      position) — the recipe of profiles/filter_form_kernels.txt.
list: the trace cut at the markers -> "label: kernels in launch order", names without namespace and parameter list."""
import csv
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(labels_path, forms=False):
    import numpy as np
    import torch

    from quadrupedal_foothold_planner_amd.planner import FootholdPlanner
    from tests import elevation_update_reference as er
    from tests import filter_form_cases
    from tests.test_cpu_filter_route import FALLBACKS, TABLE

    if forms:
        cases = [(c.label, (c.rows, c.cols, c.res, c.radii, (5, 3), c.pos)) for c in filter_form_cases.CASES]
    else:
        cases = [(label, c[:5] + ((0.0, 0.0),)) for label, c in list(TABLE.items()) + list(FALLBACKS.items())]
    p = FootholdPlanner(0)
    marker = torch.zeros(64, device="cuda")
    labels = []
    for label, (rows, cols, res, radii, shift, pos0) in cases:
        fp = p.filter_params(**radii)
        e0 = er.terrain(rows, cols, 5)
        pos1 = er.moved_position(pos0, shift, res)
        pv = er.patch_values([(30, 14, 4, 4)], 6)
        d_e = torch.from_numpy(np.ascontiguousarray(er.compose_elevation(e0, shift, pv))).cuda()
        d_t = torch.empty(rows * cols, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        marker.fill_(1.0)
        torch.cuda.synchronize()
        p.traversability_device(d_e.data_ptr(), d_t.data_ptr(), rows, cols, res, position=pos1, params=fp)
        torch.cuda.synchronize()
        labels.append(label + " | chain")
        p.gridmapCallback(np.zeros((rows, cols), np.float32), e0, res, position=pos0)
        marker.fill_(2.0)
        torch.cuda.synchronize()
        info = p.update_elevation(shift, pos1, pv, params=fp)
        torch.cuda.synchronize()
        labels.append(label + f" | update route {info['route']}")
    p.close()
    with open(labels_path, "w") as f:
        f.write("\n".join(labels) + "\n")


def listing(trace_path, labels_path):
    rows = sorted(csv.DictReader(open(trace_path)), key=lambda r: int(r["Dispatch_Id"]))
    labels = open(labels_path).read().splitlines()
    segs, cur = [], None
    for r in rows:
        name = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "")
        if "at::native" in name and "ill" in name:  # a marker
            cur = []
            segs.append(cur)
        elif cur is not None and "filter_" in name:
            cur.append(re.sub(r"\(.*", "", name).replace("fpe::", "").replace(" ", ""))
    if len(segs) == len(labels) + 1:  # (the fill that created the marker itself)
        segs = segs[1:]
    assert len(segs) == len(labels), (len(segs), len(labels))
    for lab, seg in zip(labels, segs):
        print(f"{lab}: {' '.join(seg)}")


if __name__ == "__main__":
    if sys.argv[1] in ("run", "run-forms"):
        run(sys.argv[2], forms=sys.argv[1] == "run-forms")
    else:
        listing(sys.argv[2], sys.argv[3])
