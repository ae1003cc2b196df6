#!/bin/bash
# Build libsmhip with extra compiler flags into tools/bin/<name>.so: this is where an experiment lives -- as flags on this
# command line, not as #if code in the product.  SMHIP_LIBRARY=<that file> makes the Python binding load it.  The sources and
# the flags are simplemath_amd/build.py's (SOURCES, FLAGS); the extra flags follow them.
# usage: tools/build_variant.sh ft512 -DSMHIP_FLAT_TILE_THREADS=512   |   tools/build_variant.sh preload -mllvm -amdgpu-kernarg-preload-count=16
set -e
name=$1; shift
root=$(cd "$(dirname "$0")/.." && pwd)
out=$root/tools/bin/obj_$name
rm -rf $out; mkdir -p $out  # (no object of an earlier build of this name can reach the link)
cd $root
{ read -r hipcc; read -r flags; read -r sources; } < <(python3 -c "
from simplemath_amd import build
build._generate_jit_sources()
print(build.HIPCC); print(' '.join(build.FLAGS)); print(' '.join(build.SOURCES))") || true
[ -n "$sources" ] || { echo "could not read simplemath_amd/build.py" >&2; exit 1; }
objs=; pids=
for f in $sources; do
  o=$out/${f%.hip}.o; objs="$objs $o"
  while [ "$(jobs -rp | wc -l)" -ge "${MAX_JOBS:-4}" ]; do sleep 1; done
  $hipcc $flags "$@" -c $root/simplemath_amd/csrc/$f -o $o &
  pids="$pids $!"
done
for p in $pids; do wait $p; done  # every compile's own status: a failed one stops the script here
$hipcc -shared -fPIC --offload-arch=gfx950 -o $root/tools/bin/$name.so $objs -lhiprtc -ldl
echo built $root/tools/bin/$name.so
