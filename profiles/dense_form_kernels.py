"""Which kernels the open-loop queries, the dense maps and the layer export launch, per case of tests/dense_form_cases.py — the recipe
of profiles/dense_form_kernels.txt.

    rocprofv3 --kernel-trace --output-format csv -d OUT -o dense -- python3 profiles/dense_form_kernels.py run OUT/labels.txt
    python3 profiles/dense_form_kernels.py list OUT/dense_kernel_trace.csv OUT/labels.txt

run:  the one call of every case (dense_form_cases.call, on the case's own map, parameters and tuning), each behind a marker kernel
      (a torch fill); the labels, in order, go to the file named.  One process, no counters.
list: the trace cut at the markers -> "label: kernels in launch order", names without namespace, blanks and parameter list.  Only
      the kernels of the six launch functions and of the export are listed (the upload's canonicalisation and the bit planes'
      build are not theirs)."""
import csv
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FAMILIES = ("search_legs_kernel", "centroid_legs_kernel", "footmap_", "footsnap_", "cmap_", "layers_export_kernel")


def run(labels_path):
    import torch

    from quadrupedal_foothold_planner_amd.planner import FootholdPlanner
    from tests import dense_form_cases as dc

    p = FootholdPlanner(0)
    marker = torch.zeros(64, device="cuda")
    labels = []
    for k, case in enumerate(dc.CASES):
        dc.upload(p, case)
        torch.cuda.synchronize()
        marker.fill_(float(k))
        torch.cuda.synchronize()
        dc.call(p, case)
        torch.cuda.synchronize()
        labels.append(case.label)
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
            continue
        name = re.sub(r"\(.*", "", name).replace("fpe::", "").replace(" ", "")
        if cur is not None and name.startswith(FAMILIES):
            cur.append(name)
    if len(segs) == len(labels) + 1:  # (the fill that created the marker itself)
        segs = segs[1:]
    assert len(segs) == len(labels), (len(segs), len(labels))
    for lab, seg in zip(labels, segs):
        print(f"{lab}: {' '.join(seg)}")


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2])
    else:
        listing(sys.argv[2], sys.argv[3])
