#!/bin/bash
# Build libdemfi_hip.so for gfx950 (MI355X).  hipcc cross-compiles without a GPU.
set -e
cd "$(dirname "$0")"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -I../../include -Wno-unused-result -Wno-pass-failed -Werror=inline-asm -Werror=unused-value"
# the trace build (--trace below) takes extra flags from the environment; the product compile line is fixed
XFLAGS="$DEMFI_EXTRA_FLAGS"
# conv.hip = the dispatcher (demfi_conv2d); the convolution kernels are units of their own (round 6: they compile in parallel, 2 min -> 1 min)
CONV_UNITS="conv conv_general conv_c64 conv_narrow conv_sep conv_wstream"
SRCS_HIP="pointwise.hip"
for u in $CONV_UNITS; do SRCS_HIP="$SRCS_HIP $u.hip"; done
# the host units, ONE list: the product compile loop and the --asan branch below both run over it.  abi.cpp = ABI glue; ctx.cpp = context
# life cycle + op interpreter; plan.cpp = launch plan; layout.cpp = workspace layout + arena; conv_build.cpp = descriptor builder;
# png_codec.cpp parses untrusted bytes
HOST_UNITS="abi ctx plan layout conv_build png_codec"
[ -f metrics.hip ] && SRCS_HIP="$SRCS_HIP metrics.hip"
[ -f fgac_window.hip ] && SRCS_HIP="$SRCS_HIP fgac_window.hip"
[ -f resblock.hip ] && SRCS_HIP="$SRCS_HIP resblock.hip"
[ -f gru.hip ] && SRCS_HIP="$SRCS_HIP gru.hip"
[ -f viz.hip ] && SRCS_HIP="$SRCS_HIP viz.hip"
[ -f yuv.hip ] && SRCS_HIP="$SRCS_HIP yuv.hip"
[ -f frames16.hip ] && SRCS_HIP="$SRCS_HIP frames16.hip"
[ -f yuv_family.hip ] && SRCS_HIP="$SRCS_HIP yuv_family.hip"
[ -f tile.hip ] && SRCS_HIP="$SRCS_HIP tile.hip"
[ -f dedup.hip ] && SRCS_HIP="$SRCS_HIP dedup.hip"
[ -f deint.hip ] && SRCS_HIP="$SRCS_HIP deint.hip"
[ -f wsconv.hip ] && SRCS_HIP="$SRCS_HIP wsconv.hip"
# stale objects must never be linked: a failed compile has to fail the build
rm -f ./*.o libdemfi_hip.so
pids=()
objs=()
# conv.hip: no SLP vectorisation -- the auto-packed v_pk_add_f32 of the epilogues need v_mov shuffles around the accumulator
# registers (250 instead of 128 VALU in the 64->64 epilogue) and packed f32 VALU is slow beside MFMAs (MI355X_MICROARCH.md)
CONV_FLAGS="-fno-slp-vectorize"
for s in $SRCS_HIP; do
  o="${s%.hip}.o"; objs+=("$o")
  xf=""; case "$s" in conv*.hip|resblock.hip|gru.hip|wsconv.hip) xf="$CONV_FLAGS" ;; esac
  $HIPCC $FLAGS $xf -c "$s" -o "$o" & pids+=($!)
done
for u in $HOST_UNITS; do
  objs+=("$u.o")
  $HIPCC $FLAGS -x hip -c "$u.cpp" -o "$u.o" & pids+=($!)
done
for p in "${pids[@]}"; do wait "$p"; done      # 'wait PID' returns that job's status: set -e stops on the first failure
$HIPCC --offload-arch=gfx950 -shared -fPIC "${objs[@]}" -o libdemfi_hip.so -lz -lpthread
echo "built $(pwd)/libdemfi_hip.so"
# --trace: second library whose persistent 64->64 kernels stamp s_memtime at their phase boundaries (tools/phase_trace.py)
if [ "$1" = "--trace" ]; then
  tp=()
  for u in $CONV_UNITS gru resblock; do
    $HIPCC $FLAGS $XFLAGS $CONV_FLAGS -DDEMFI_TRACE -c $u.hip -o ${u}_trace.o & tp+=($!)
  done
  for p in "${tp[@]}"; do wait "$p"; done
  trc=()
  for o in "${objs[@]}"; do
    case "$o" in conv*.o|resblock.o|gru.o) trc+=("${o%.o}_trace.o") ;; *) trc+=("$o") ;; esac
  done
  $HIPCC --offload-arch=gfx950 -shared -fPIC "${trc[@]}" -o libdemfi_hip_trace.so -lz -lpthread
  echo "built $(pwd)/libdemfi_hip_trace.so"
fi
# --asan: host-side AddressSanitizer + UBSan build: every host unit of HOST_UNITS instrumented, linked with the
# ordinary kernel objects.  tools/asan_check.sh does NOT use this library: it builds its own, with ctx.cpp, abi.cpp and png_codec.cpp
# instrumented only (plan.cpp, layout.cpp, conv_build.cpp plain); those three run under the sanitizers in tests/c/plan_walk_san.sh.
if [ "$1" = "--asan" ]; then
  # pointer-overflow is off on purpose: the sizing pass of demfi_ctx_create lays the plan out on a NULL base (addresses == workspace offsets)
SAN="-O1 -g -fsanitize=address,undefined -fno-sanitize=pointer-overflow -fno-gpu-sanitize -fno-omit-frame-pointer -shared-libsan -fno-sanitize-recover=undefined"
  aso=()
  for o in "${objs[@]}"; do
    u="${o%.o}"
    if [[ " $HOST_UNITS " == *" $u "* ]]; then
      $HIPCC --offload-arch=gfx950 -std=c++17 -fPIC -ffp-contract=off -I../../include -Wno-unused-result $SAN -x hip -c "$u.cpp" -o "${u}_asan.o"
      aso+=("${u}_asan.o")
    else aso+=("$o"); fi
  done
  $HIPCC --offload-arch=gfx950 -shared -fPIC -fsanitize=address,undefined -fno-gpu-sanitize -shared-libsan "${aso[@]}" -o libdemfi_hip_asan.so -lz -lpthread
  echo "built $(pwd)/libdemfi_hip_asan.so"
fi
