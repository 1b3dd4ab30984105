#!/bin/bash
# Builds oracle/_ref/ from the reference sources WHERE THEY LIE under /root/reference.
# TEST INFRASTRUCTURE: outputs only into oracle/_ref/ (git-ignored, but it travels to the GPU box).
#   ref_host_dump_O0 : the reference's host classes (Model, AccelerationStructureExplicit,
#       Camera, Resource) + oracle/ref_host_dump.cpp, compiled with g++ directly (no cmake),
#       unoptimised like the reference CI (no CMAKE_BUILD_TYPE).
#   <kernel>.strict.co / <kernel>.default.co : the reference's own OpenCL kernels compiled for
#       gfx950 by the image's ROCm clang with the image's real OpenCL device libraries -- what
#       clBuildProgram would produce on the MI355X.  "strict" = -ffp-contract=off
#       -cl-fp32-correctly-rounded-divide-sqrt (the floating-point model oracle/lt_oracle.c
#       restates); "default" = what NULL build options give (renderer_opencl.cpp:50).
#   math_probe.strict.co / math_probe.default.co : oracle/math_probe.cl, the project's own probe of the OpenCL builtins and
#       operators, compiled the same two ways.  Needs no reference tree: built (when its source is newer) before anything else.
# The reference-derived part is a no-op (exit 0) when /root/reference is absent (the GPU box uses the prebuilt files).
set -e
REF=${LT_REFERENCE_DIR:-/root/reference}
HERE=$(cd "$(dirname "$0")" && pwd)
OUT=$HERE/_ref
mkdir -p "$OUT"
CLANG=${LT_OPENCL_CLANG:-/opt/rocm/lib/llvm/bin/clang}
CLFLAGS="-x cl -cl-std=CL2.0 -target amdgcn-amd-amdhsa -mcpu=gfx950 -Xclang -finclude-default-header -O3 -w"
STRICT="-ffp-contract=off -cl-fp32-correctly-rounded-divide-sqrt"
if [ "$OUT/math_probe.default.co" -ot "$HERE/math_probe.cl" ] || [ "$OUT/math_probe.strict.co" -ot "$HERE/math_probe.cl" ]; then
  $CLANG $CLFLAGS $STRICT "$HERE/math_probe.cl" -o "$OUT/math_probe.strict.co"
  $CLANG $CLFLAGS "$HERE/math_probe.cl" -o "$OUT/math_probe.default.co"
fi
if [ ! -d "$REF/src" ]; then echo "build_ref: $REF not present, keeping prebuilt oracle/_ref"; exit 0; fi
for opt in O0; do
  g++ -std=c++17 -$opt -w -I"$REF/include" "$HERE/ref_host_dump.cpp" \
      "$REF/src/model.cpp" "$REF/src/acceleration_structure_explicit.cpp" "$REF/src/camera.cpp" "$REF/src/resource.cpp" \
      -o "$OUT/ref_host_dump_$opt"
done
declare -A K=(
  [basic]=resources/kernels/opencl/basic.cl
  [basic_lighting]=resources/kernels/opencl/basic_lighting.cl
  [accumulator]=examples/accumulator/resources/kernels/accumulator.cl
  [global_illumination]=examples/global_illumination/resources/kernels/global_illumination.cl
  [global_illumination25]=resources/kernels/opencl/global_illumination.cl
  [custom_opencl]=examples/custom_kernel/resources/kernels/custom_opencl.cl
)
for name in "${!K[@]}"; do
  src="$REF/${K[$name]}"
  $CLANG $CLFLAGS $STRICT "$src" -o "$OUT/$name.strict.co"
  $CLANG $CLFLAGS "$src" -o "$OUT/$name.default.co"
done
ls -la "$OUT"
