#!/usr/bin/env python3
"""What the refinement decision costs where the level's image lies in device memory: bl_adaptive_refine_device (one kernel, the flags
come down) beside the path it replaces on the same box - the image copied to pageable host memory and decided by bl_adaptive_refine.
Writes profiles/refine_device.json.

    python tools/gpu_refine_device.py [--out profiles/refine_device.json] [--resolution 2048] [--block 8] [--refined-blocks 10000]

One level of --resolution^2 pixels in blocks of --block^2, random finite pixels, the row layouts of the fixtures sim_adaptive (1 image
row) and sim_polarized_adaptive (5 rows); every criterion alone and all five, with cuts nothing exceeds, so that no block refines and
every criterion that is on walks every block (the worst case); and one refined level of --refined-blocks blocks with all five. For
each: the device call's wall time (median, min, max of five calls after a first), the same of the replaced path (download +
bl_adaptive_refine) and of its two halves, and whether flags and lists were equal. The measuring runs in one child process under
`timeout -k 10`; a failure ends the job. No time is a pass / fail condition."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CRITERIA = ("val", "abs_grad", "rel_grad", "abs_lapl", "rel_lapl")


def _spread(ms):
    return dict(ms_median=statistics.median(ms), ms_min=min(ms), ms_max=max(ms), calls=len(ms))


def measure(args):
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import numpy as np
    import torch
    import blacklight_amd as bl
    import golden_util as gu
    torch.cuda.set_device(0)
    res, bs = args.resolution, args.block
    rng = np.random.default_rng(2048)
    for case in ("sim_adaptive", "sim_polarized_adaptive"):
        for on in [(name,) for name in CRITERIA] + [CRITERIA]:
            for level in ((0, 1) if on == CRITERIA else (0,)):
                fx, params, _ = gu.load_case(case)
                for key in [k for k in params if k.startswith("adaptive_region_")]:
                    params.pop(key)
                params.update(camera_resolution=res, adaptive_block_size=bs, adaptive_max_level=2, adaptive_num_regions=0)
                for name in CRITERIA:
                    params[f"adaptive_{name}_cut"] = 1.0e30
                    params[f"adaptive_{name}_frac"] = 0.5 if name in on else -1.0
                with bl.Context(bl.Params.from_dict(params), device=0) as ctx:
                    rows = ctx.num_quantities
                    locs = None
                    if level == 1:
                        side = 2 * (res // bs)
                        chosen = rng.permutation(side * side)[: args.refined_blocks]
                        locs = np.stack([chosen // side, chosen % side], axis=1).astype(np.int32)
                    pixels = res * res if level == 0 else locs.shape[0] * bs * bs
                    image = torch.from_numpy(rng.uniform(0.1, 1.0, (rows, pixels))).cuda()
                    torch.cuda.synchronize()
                    device_ms, host_ms, copy_ms, decide_ms = [], [], [], []
                    equal = True
                    for call in range(6):
                        t0 = time.perf_counter()
                        flags, nxt = ctx.adaptive_refine_device(level, image, locs)
                        t1 = time.perf_counter()
                        on_host = image.cpu().numpy()   # (pageable memory, as Context.render's own arrays)
                        t2 = time.perf_counter()
                        want_flags, want_next = ctx.adaptive_refine(level, on_host, locs)
                        t3 = time.perf_counter()
                        equal = equal and bool(np.array_equal(flags, want_flags) and np.array_equal(nxt, want_next))
                        if call > 0:   # (the first call allocates the context's scratch and touches the pages)
                            device_ms.append(1000.0 * (t1 - t0))
                            copy_ms.append(1000.0 * (t2 - t1))
                            decide_ms.append(1000.0 * (t3 - t2))
                            host_ms.append(1000.0 * (t3 - t1))
                    print(json.dumps(dict(layout=case, image_rows=rows, level=level, n_blocks=int(flags.shape[0]), block_size=bs, criteria=list(on),
                                          device_call=_spread(device_ms), replaced_path=_spread(host_ms), replaced_path_download=_spread(copy_ms),
                                          replaced_path_host_decision=_spread(decide_ms), flags_and_lists_equal=equal, blocks_refined=int(flags.sum()))),
                          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "refine_device.json"))
    ap.add_argument("--resolution", type=int, default=2048)
    ap.add_argument("--block", type=int, default=8)
    ap.add_argument("--refined-blocks", type=int, default=10000)
    ap.add_argument("--step", choices=["measure"], default=None, help="(internal) measure in this process")
    args = ap.parse_args()
    if args.step == "measure":
        return measure(args)
    command = [sys.executable, os.path.abspath(__file__), "--step", "measure", "--resolution", str(args.resolution), "--block", str(args.block),
               "--refined-blocks", str(args.refined_blocks)]
    run = subprocess.run(["timeout", "-k", "10", "300"] + command, cwd=REPO, capture_output=True, text=True)
    if run.returncode != 0:
        sys.stderr.write(run.stdout[-4000:] + run.stderr[-4000:])
        sys.exit(f"measuring failed with status {run.returncode}")
    result = dict(what=f"bl_adaptive_refine_device beside download + bl_adaptive_refine: {args.resolution}^2 pixels, blocks of {args.block}^2, one GPU; "
                       "wall times of the calls in ms, five calls after a first",
                  configurations=[json.loads(line) for line in run.stdout.splitlines() if line.startswith("{")])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
