"""The bookkeeping of the two library queues (simplemath_amd/csrc/queue_order.h, the code runtime.hip runs), compiled for the
host with the address and undefined-behaviour sanitizers and driven by tests/cpp/queue_order_host.cpp with an `order` that only
records "queue q waits for queue p".  A model with its own operator counts checks happens-before for every pair of
conflicting operators (overlapping bytes, one of them writing; barrier operators, external waits and synchronises included)
over random programs, over directed programs in which a record falls out of the table without one edge on the way, and over
precision programs in which independent work must make no edge at all."""
import re
import subprocess

MIN_SPAN_PAIRS = 10 ** 6  # conflicting pairs of operators with declared spans; pairs with a barrier operator come on top


def test_queue_order_orders_every_conflicting_pair_on_host():
    from simplemath_amd import build
    exe = build.build_host_programs()["queue_order_host"]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    m = re.search(r"queue_order ok operators (\d+) pairs (\d+) span_pairs (\d+): (\d+) unordered", r.stdout)
    assert m, r.stdout[-3000:]
    assert int(m.group(3)) >= MIN_SPAN_PAIRS and int(m.group(2)) >= int(m.group(3)), r.stdout[-3000:]
    assert int(m.group(4)) == 0, r.stdout[-3000:]
    e = re.search(r"eviction programs (\d+) unordered (\d+), precision (\w+)", r.stdout)
    assert e and int(e.group(1)) == 6 and int(e.group(2)) == 0 and e.group(3) == "ok", r.stdout[-3000:]
