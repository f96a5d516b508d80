#!/bin/bash
# Diagnostic build with in-kernel phase stamps (never shipped, never timed): libi2lqr_stamps.so.
# A translation unit that does not compile with the stamps (the wave / lane kernels' units trip a
# code generator assertion on some compiler builds) falls back to the product object, so the
# stamps of the other kernel families stay usable.  The units are the Makefile's (make units).
cd "$(dirname "$0")/../ilqr_iterative_tasks_amd/csrc" || exit 1
make -s >/dev/null 2>&1
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -DI2LQR_STAMPS ${EXTRA:-}"  # EXTRA: experiment switches
objs=""
for tu in $(make -s units); do
  ( /opt/rocm/bin/hipcc $FLAGS -c -o /tmp/${tu}_st.o ${tu}.hip >/tmp/${tu}_st.log 2>&1 \
      || { echo "stamps: ${tu}.hip does not build with -DI2LQR_STAMPS, using the product object"; \
           cp _obj/${tu}.o /tmp/${tu}_st.o; } ) &
  objs="$objs /tmp/${tu}_st.o"
done
wait
set -e
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -o /tmp/libi2lqr_stamps.so $objs
mkdir -p ../../tools/_diag && cp /tmp/libi2lqr_stamps.so ../../tools/_diag/libi2lqr_stamps.so
ls -la ../../tools/_diag/libi2lqr_stamps.so
