"""HBM traffic of the new rows of tools/unary_rates.py from rocprofv3 PMC counters, against the algorithmic bytes.
FETCH_SIZE and WRITE_SIZE are collected in runs of their own:

    rocprofv3 --pmc FETCH_SIZE --output-format csv -d DIR/fetch -- python tools/unary_rates.py --single
    rocprofv3 --pmc WRITE_SIZE --output-format csv -d DIR/write -- python tools/unary_rates.py --single
    python tools/unary_pmc.py DIR

Dispatches are assigned to the rows in order: the measured call of each row sits between two marker fills (the copies that
build the operands come before the first).  Counters are in KiB; FETCH_SIZE reports half the bytes of a 16-byte-per-lane streaming read on gfx950
(tools/axis_reduce_pmc.py), so the read bytes are given raw and doubled."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from axis_reduce_pmc import dispatches, per_case  # noqa: E402
from unary_rates import table  # noqa: E402


def main():
    d = sys.argv[1]
    fetch, write = per_case(dispatches(os.path.join(d, "fetch"), "FETCH_SIZE"))[0::2], per_case(dispatches(os.path.join(d, "write"), "WRITE_SIZE"))[0::2]
    print("%-30s %-44s %10s %10s %10s %10s %9s" % ("row (one call)", "kernels", "alg MiB", "FETCH raw", "FETCH x2", "WRITE", "x2+W/alg"))
    for row, f, w in zip(table(), fetch, write):
        alg = row[1] / 2 ** 20
        fr, wr = sum(v for _, v in f) / 1024.0, sum(v for _, v in w) / 1024.0
        names = ",".join(sorted({n.split("<")[0].split("(")[0].replace("void smhip::", "").replace("(anonymous namespace)::", "") for n, _ in f}))
        print("%-30s %-44s %10.1f %10.1f %10.1f %10.1f %9.3f" % (row[0], names[:44], alg, fr, 2 * fr, wr, (2 * fr + wr) / alg))


if __name__ == "__main__":
    main()
