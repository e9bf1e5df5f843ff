#!/usr/bin/env python
"""Records tests/golden/voxel_metrics_table.npz and voxel_metrics_table_<i>.csv: the metrics table of the reference
project for the confusion matrices cm_0 .. cm_4 of tests/golden/metrics.npz (an absent class, a never-hit class and a
void-only ground truth are among them), and the CSV pandas writes for it.

  python tools/gen_voxel_metrics_golden.py        (needs the reference's sources and pandas; CPU only)

The numbers come from the reference's own voxel_metrics.compute_tfpn, compute_tfpn_fg and compute_voxel_metrics, imported
from CORENET_REFERENCE (default /root/reference/src).  Its evaluation_results module cannot be imported without
TensorBoard and the rest of its pipeline, so the frame is put together here the way evaluation_results.py:203-210 and :269
describe: one frame of the per-class metrics indexed by the class names and transposed, one of the foreground /
background metrics under "__global__", joined along the columns, then DataFrame.to_csv.  No test runs this script; the
tests read what it wrote."""
import dataclasses
import io
import os
import sys
import types

import numpy as np
import pandas
import torch as t

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.environ.get("CORENET_REFERENCE", "/root/reference/src"))
_stub = types.ModuleType("dataclasses_jsonschema")            # not installed; nothing here calls it
_stub.JsonSchemaMixin = type("JsonSchemaMixin", (), {})
sys.modules.setdefault("dataclasses_jsonschema", _stub)

from corenet import voxel_metrics                             # noqa: E402  (the reference)


def class_names(k: int):
  names = ["__void__"] + [f"c{j}" for j in range(1, k)]
  if k == 5:
    names[2] = "sofa, couch"                                  # a name the CSV has to quote
  return names


def frame(vm, index):
  return pandas.DataFrame({f.name: np.atleast_1d(getattr(vm, f.name).numpy()) for f in dataclasses.fields(vm)}, index=index).T


def main():
  src = np.load(os.path.join(GOLDEN, "metrics.npz"))
  out = {}
  for i in range(5):
    cm = t.from_numpy(src[f"cm_{i}"])
    names = class_names(cm.shape[0])
    per_class = voxel_metrics.compute_voxel_metrics(voxel_metrics.compute_tfpn(cm))
    fg = voxel_metrics.compute_voxel_metrics(voxel_metrics.compute_tfpn_fg(cm))
    df = pandas.concat([frame(per_class, names), frame(fg, ["__global__"])], axis=1)
    assert list(df.index) == ["iou", "precision", "recall"]
    miou = float(df.iloc[:, 1:-1].T.mean().iou)
    recorded = float(src[f"miou_{i}"])
    assert (np.isnan(miou) and np.isnan(recorded)) or miou == recorded, (i, miou, recorded)
    df.to_csv(fl := io.StringIO())
    with open(os.path.join(GOLDEN, f"voxel_metrics_table_{i}.csv"), "w", newline="") as f:
      f.write(fl.getvalue())
    out[f"table_{i}"] = df.to_numpy(dtype=np.float64)
    out[f"classes_{i}"] = np.array(names)
    tfpn = voxel_metrics.compute_tfpn(cm)
    out[f"tfpn_{i}"] = np.stack([getattr(tfpn, k).numpy() for k in ("tp", "tn", "fp", "fn")])
    tfg = voxel_metrics.compute_tfpn_fg(cm)
    out[f"tfpn_fg_{i}"] = np.array([int(getattr(tfg, k)) for k in ("tp", "tn", "fp", "fn")])
  np.savez_compressed(os.path.join(GOLDEN, "voxel_metrics_table.npz"), **out)
  print("voxel metrics goldens written to", GOLDEN)


if __name__ == "__main__":
  main()
