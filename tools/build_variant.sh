#!/bin/bash
# Tuning builds (never the product): the C1/C2 register-kernel instantiations
# (gen_inst.py SOCP_DEV_VARIANTS) compiled with extra flags, linked with the
# product build's other objects into socp.jl_amd/lib/v_<name>/libsocp.so.
# The compile flags and the lists of the API units and of those objects come
# from the Makefile.
#   tools/build_variant.sh <name> "<extra hipcc flags>"
set -e
name=$1; extra=$2
R=$(cd "$(dirname "$0")/.." && pwd)
C=$R/socp.jl_amd/csrc
GEN=$R/socp.jl_amd/build/gen_v_$name
OBJ=$R/socp.jl_amd/build/obj_v_$name
LIB=$R/socp.jl_amd/lib/v_$name
mkdir -p $GEN $OBJ $LIB
export SOCP_DEV_VARIANTS=${DEV_VARIANTS:-1}
python3 $C/gen_inst.py $GEN > /dev/null
mk() { make -s --no-print-directory -C $C GEN=$GEN EXTRA="$extra" "$@"; }
HIPCC=$(mk print-HIPCC)
FLAGS=$(mk print-HIPFLAGS)
pids=()
for f in $GEN/inst_*.hip; do
  b=$(basename $f .hip)
  $HIPCC $FLAGS -c $f -o $OBJ/$b.o > $OBJ/$b.log 2>&1 &
  pids+=($!)
done
# the C ABI units too (host-side layout helpers such as small_lds_bytes see the flags)
AOBJS=
for o in $(mk print-API_OBJS); do
  b=${o%.o}
  $HIPCC $FLAGS -c $C/$b.hip -o $OBJ/$o > $OBJ/$b.log 2>&1 &
  pids+=($!)
  AOBJS="$AOBJS $OBJ/$o"
done
for p in "${pids[@]}"; do wait $p || { echo "compile failed"; cat $OBJ/*.log | tail -20; exit 1; }; done
M=$R/socp.jl_amd/build/obj
KOBJS=$(for o in $(mk print-KERNEL_OBJS); do echo $M/$o; done)
$HIPCC --offload-arch=gfx950 -shared -fPIC -o $LIB/libsocp.so $AOBJS $KOBJS $OBJ/inst_*.o
echo "built $LIB/libsocp.so"
