"""The block-to-tile mapping of long streaming launches (simplemath_amd/csrc/front_order.h, the source the gfx950 kernels
inline), compiled for the host with the address and undefined-behaviour sanitizers and checked exhaustively: a bijection on
[0, nb) for every nb from 1 to 5000, for 2^17, 2^17 + 1, 2^19 - 3 and 8 C k +- 1, for every C the library can choose; the
identity below 8 C tiles and on the ragged end."""
import re
import subprocess


def test_front_order_is_a_bijection_on_host():
    from simplemath_amd import build
    exe = build.build_host_programs()["front_order_host"]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = re.search(r"front_order ok shapes (\d+)", r.stdout)
    assert m and int(m.group(1)) >= 9 * 2 * 5000, r.stdout[-2000:]
