#!/bin/bash
# Build libdemfi_hip.so for gfx950 (MI355X).  hipcc cross-compiles without a GPU.
#   build.sh                      the product library
#   build.sh --trace              + libdemfi_hip_trace.so (phase stamps, tools/phase_trace.py, rb_trace.py, gru_trace.py)
#   build.sh --asan               + libdemfi_hip_asan.so (host units under ASan + UBSan)
#   build.sh --asm DIR [--trace]  device assembly of every HIP unit into DIR/<unit>.s, compiled exactly as the product compiles it
#                                 (--trace: DIR/<unit>_trace.s of the trace units instead); compiles and nothing else
set -e
case "$1" in --asm) mkdir -p "$2"; ASM_DIR=$(cd "$2" && pwd) ;; esac
cd "$(dirname "$0")"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -I../../include -Wno-unused-result -Wno-pass-failed -Werror=inline-asm -Werror=unused-value"
# the trace build (--trace below) takes extra flags from the environment; the product compile line is fixed
XFLAGS="$DEMFI_EXTRA_FLAGS"
# the HIP units, ONE list, in link order.  conv = the dispatcher (demfi_conv2d); the convolution kernels are units of their own (round 6:
# they compile in parallel, 2 min -> 1 min)
HIP_UNITS="pointwise conv conv_general conv_c64 conv_narrow conv_sep conv_wstream metrics fgac_window resblock gru viz yuv frames16 yuv_family tile dedup deint denoise deblock dering nlmeans deband ivtc crop shutter interlace scale bitdepth grain colour lut3d wsconv"
# the MFMA units: no SLP vectorisation -- the auto-packed v_pk_add_f32 of the epilogues need v_mov shuffles around the accumulator
# registers (250 instead of 128 VALU in the 64->64 epilogue) and packed f32 VALU is slow beside MFMAs (MI355X_MICROARCH.md)
NOSLP_UNITS="conv conv_general conv_c64 conv_narrow conv_sep conv_wstream resblock gru wsconv"
# the trace library recompiles the MFMA units that carry phase stamps: all of them but wsconv (its stamps are a kernel argument of the product)
TRACE_UNITS=${NOSLP_UNITS/ wsconv/}
# the host units, ONE list: the product compile loop and the --asan branch below both run over it.  abi.cpp = ABI glue; ctx.cpp = context
# life cycle + op interpreter; plan.cpp = launch plan; layout.cpp = workspace layout + arena; conv_build.cpp = descriptor builder;
# png_codec.cpp parses untrusted bytes
HOST_UNITS="abi ctx plan layout conv_build png_codec"
in_list() { [[ " $2 " == *" $1 "* ]]; }
# THE compile line of a HIP unit: hip_cc UNIT product|trace ARGS..., where ARGS are the output kind and the files
hip_cc() {
  local xf=""
  if [ "$2" = trace ]; then xf="$XFLAGS -fno-slp-vectorize -DDEMFI_TRACE"; elif in_list "$1" "$NOSLP_UNITS"; then xf="-fno-slp-vectorize"; fi
  shift 2
  $HIPCC $FLAGS $xf "$@"
}
pids=()
wait_all() { for p in "${pids[@]}"; do wait "$p"; done; pids=(); }     # 'wait PID' returns that job's status: set -e stops on the first failure
if [ -n "$ASM_DIR" ]; then
  if [ "$3" = "--trace" ]; then
    for u in $TRACE_UNITS; do hip_cc $u trace --cuda-device-only -S $u.hip -o "$ASM_DIR/${u}_trace.s" & pids+=($!); done
  else
    for u in $HIP_UNITS; do hip_cc $u product --cuda-device-only -S $u.hip -o "$ASM_DIR/$u.s" & pids+=($!); done
  fi
  wait_all
  exit 0
fi
# stale objects must never be linked: a failed compile has to fail the build
rm -f ./*.o libdemfi_hip.so
objs=()
for u in $HIP_UNITS; do
  objs+=("$u.o")
  hip_cc $u product -c $u.hip -o $u.o & pids+=($!)
done
for u in $HOST_UNITS; do
  objs+=("$u.o")
  $HIPCC $FLAGS -x hip -c "$u.cpp" -o "$u.o" & pids+=($!)
done
wait_all
$HIPCC --offload-arch=gfx950 -shared -fPIC "${objs[@]}" -o libdemfi_hip.so -lz -lpthread
echo "built $(pwd)/libdemfi_hip.so"
# --trace: second library whose persistent 64->64 kernels stamp s_memtime at their phase boundaries (tools/phase_trace.py)
if [ "$1" = "--trace" ]; then
  for u in $TRACE_UNITS; do hip_cc $u trace -c $u.hip -o ${u}_trace.o & pids+=($!); done
  wait_all
  trc=()
  for o in "${objs[@]}"; do
    if in_list "${o%.o}" "$TRACE_UNITS"; then trc+=("${o%.o}_trace.o"); else trc+=("$o"); fi
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
    if in_list "$u" "$HOST_UNITS"; then
      $HIPCC --offload-arch=gfx950 -std=c++17 -fPIC -ffp-contract=off -I../../include -Wno-unused-result $SAN -x hip -c "$u.cpp" -o "${u}_asan.o"
      aso+=("${u}_asan.o")
    else aso+=("$o"); fi
  done
  $HIPCC --offload-arch=gfx950 -shared -fPIC -fsanitize=address,undefined -fno-gpu-sanitize -shared-libsan "${aso[@]}" -o libdemfi_hip_asan.so -lz -lpthread
  echo "built $(pwd)/libdemfi_hip_asan.so"
fi
