"""HBM traffic of the axis-reduction rate table (tools/axis_reduce_rates.py) from rocprofv3 PMC counters, against the
algorithmic bytes (input + output).  FETCH_SIZE and WRITE_SIZE are collected in separate runs of their own:

    rocprofv3 --pmc FETCH_SIZE --output-format csv -d DIR/fetch -- python tools/axis_reduce_rates.py --steps 1 --warmup 0 --kinds sum
    rocprofv3 --pmc WRITE_SIZE --output-format csv -d DIR/write -- python tools/axis_reduce_rates.py --steps 1 --warmup 0 --kinds sum
    python tools/axis_reduce_pmc.py DIR

Dispatches are assigned to the table's rows in order: each row starts with the fill of its input.  Counters are in KiB;
per the gfx950 notes of MI355X_MICROARCH.md FETCH_SIZE reports half the bytes of a 16-byte-per-lane streaming read, so the
read bytes are given raw and doubled."""
import csv
import glob
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from axis_reduce_rates import TABLE  # noqa: E402

FILLS = ("uniform_f32_kernel", "fill_vec_kernel")


def dispatches(dirname, counter):
    rows = {}
    for f in glob.glob(os.path.join(dirname, "**", "*counter_collection.csv"), recursive=True):
        with open(f) as fh:
            for r in csv.DictReader(fh):
                if r.get("Counter_Name") == counter:
                    key = int(r["Dispatch_Id"])
                    name, val = r["Kernel_Name"], float(r["Counter_Value"])
                    rows[key] = (name, rows.get(key, (name, 0.0))[1] + val)
    return [rows[k] for k in sorted(rows)]


def per_case(ds):
    cases, cur = [], None
    for name, val in ds:
        if any(f in name for f in FILLS):
            cur = []
            cases.append(cur)
        elif cur is not None:
            cur.append((name, val))
    return cases


def main():
    d = sys.argv[1]
    fetch, write = per_case(dispatches(os.path.join(d, "fetch"), "FETCH_SIZE")), per_case(dispatches(os.path.join(d, "write"), "WRITE_SIZE"))
    print("%-38s %6s %11s %11s %11s %11s %8s" % ("shape (sum, one call)", "kernels", "alg MiB", "FETCH raw", "FETCH x2", "WRITE", "x2+W/alg"))
    for (label, shape, dt, axes, transposed), f, w in zip(TABLE, fetch, write):
        n = int(np.prod(shape))
        ax = (axes,) if isinstance(axes, int) else axes
        sh = shape[::-1] if transposed else shape
        out_n = int(np.prod([e for k, e in enumerate(sh) if k not in ax]))
        alg = (n + out_n) * np.dtype(dt).itemsize / 2 ** 20
        fr = sum(v for _, v in f) / 1024.0
        wr = sum(v for _, v in w) / 1024.0
        print("%-38s %6d %11.1f %11.1f %11.1f %11.1f %8.3f" % (label, len(f), alg, fr, 2 * fr, wr, (2 * fr + wr) / alg))


if __name__ == "__main__":
    main()
