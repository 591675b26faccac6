"""Generates tests/golden/train_random_<seed>.npz by RUNNING the reference's own Counter.update_by_output
(LoG/model/counter.py:36-68) and SparseOptimizer.step (LoG/model/sparse_optimizer.py:163-196), unpatched, on CPU, on the
inputs of tests/train_util.py:random_case(seed) (build container only: needs the reference tree).  Stored: the counter
fields, every view's flag_vis / index_vis, the learning rates the optimizer used, the final parameters and moments.

    LOG_REFERENCE=<LoG checkout> python tests/golden/make_golden_train_random.py
"""
import io
import os
import sys
import zipfile

import numpy as np
import torch

REF = os.environ["LOG_REFERENCE"]          # a checkout of the reference (LoG)
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (REF, ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from LoG.model.counter import Counter                      # noqa: E402  reference code, imported not copied
from LoG.model.sparse_optimizer import SparseOptimizer     # noqa: E402
import train_util as U                                     # noqa: E402

SEEDS = range(6)


def case(seed):
    c = U.random_case(seed)
    out = {"P": np.int32(c["P"]), "n_views": np.int32(len(c["views"])), "n_steps": np.int32(len(c["steps"]))}
    counter = Counter(num_points=c["P"])
    o = U.random_counter_output(c["views"])
    counter.update_by_output(o, fix_parent=True)
    for k in U.COUNTER_DTYPES:
        out["counter_" + k] = getattr(counter, k).numpy()
    for v in range(len(c["views"])):
        out[f"v{v}_flag_vis"] = o["visibility_flag"][v]["flag_vis"].numpy()
        out[f"v{v}_index_vis"] = o["visibility_flag"][v]["index_vis"].numpy()
    model = c["init_model"]()
    opt = SparseOptimizer(list(c["shapes"]), dict(U.RANDOM_LR), model, device=torch.device("cpu"), xyz_scale=1.0,
                          use_amsgrad=c["amsgrad"])
    opt.global_steps += c["start_steps"]
    out["start_global_steps"] = np.float64(float(opt.global_steps))
    for k in ("colors", "shs", "opacity", "rotation"):
        out["lr_" + k] = np.float64(opt.lr_dict[k])
    for it, st in enumerate(c["steps"]):
        n = int(float(opt.global_steps)) + 1                # the step number the update uses
        out[f"s{it}_step"] = np.int64(n)
        out[f"s{it}_lr_xyz"] = np.float64(opt.xyz_scheduler_args(n))
        out[f"s{it}_lr_scaling"] = np.float64(opt.scaling_scheduler_args(n))
        opt.step(model, st["index"], U.random_step_params(model, st, c["shapes"]), st["flag_vis"])
    out["final_global_steps"] = np.float64(float(opt.global_steps))
    out["final_xyz_lr"] = np.float64(opt.xyz_lr if opt.xyz_lr is not None else np.nan)
    for k in c["shapes"]:
        out["final_" + k] = getattr(model, k).numpy()
        out["final_exp_avg_" + k] = opt.exp_avg[k].numpy()
        out["final_exp_avg_sq_" + k] = opt.exp_avg_sq[k].numpy()
        if c["amsgrad"]:
            out["final_max_exp_avg_sq_" + k] = opt.max_exp_avg_sq[k].numpy()
    return out


def save_lzma(path, arrays):
    """np.savez with LZMA members (np.load reads them like deflated ones)."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_LZMA) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.save(buf, np.asanyarray(a))
            z.writestr(name + ".npy", buf.getvalue())


def main():
    for seed in SEEDS:
        path = os.path.join(HERE, "train_random_%d.npz" % seed)
        save_lzma(path, case(seed))
        print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
