"""Long streaming launches walk their tiles in front_order.h's order ('Very large arrays'): class
blockIdx.x % 8 takes C consecutive tiles out of every group of 8 C.  The library's own rule switches it on above 2^25 vectors
per operand; SMHIP_FRONT_LOG2C=1 makes it live for every launch of the 1024-thread kernel, so that front_order_probe.py can
run it at 2^20 vectors: add for f32 / f64 / i32 / i64, a * s and the fused add+sum for f32, bit for bit against the oracle, at
n_vec = 2^20, 2^20 + 1, k G 1024 - 1, k G 1024, k G 1024 + 1 (the first k past 2^20) and 2^20 + 3 G 1024 + 517, each with
element tails of 0, 1 and W - 1 -- alone, and with SMHIP_PIECE_LOG2VEC=14 (pieces of one group each) on top."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("pieces", [None, "14"], ids=["one_launch", "pieces_of_2p14"])
def test_front_order_results_match_the_oracle(pieces):
    probe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "front_order_probe.py")
    env = dict(os.environ, SMHIP_FRONT_LOG2C="1")
    env.pop("SMHIP_PIECE_LOG2VEC", None)
    if pieces:
        env["SMHIP_PIECE_LOG2VEC"] = pieces
    r = subprocess.run([sys.executable, probe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "front_order_probe ok 126" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
