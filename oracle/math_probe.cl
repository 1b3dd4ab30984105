// Probe of the OpenCL builtins and operators the render kernels lean on, written from the OpenCL C specification.
// TEST INFRASTRUCTURE: oracle/build_ref.sh compiles it for gfx950 exactly as it compiles the reference's kernel files, once with
// NULL build options (math_probe.default.co) and once with -ffp-contract=off -cl-fp32-correctly-rounded-divide-sqrt
// (math_probe.strict.co); oracle/ref_gpu.py:probe() runs an entry point over 1-D arrays.  The results are the ground truth
// lens_trace_amd/csrc/lt_device.hpp's hand restatements (Math<1>, Math<2>, normalize4, distance4, dot4, dot2, cross4) are held
// against, bit for bit (tests/test_gpu_math_edges.py).
//
// Every kernel reads `n` records of raw bit patterns (uint per float, two uints -- low word first -- per double) from `in`
// and writes the result's bit patterns to `out`; work-item i handles record i.  Each contraction shape is ONE source expression,
// as the expressions it stands for are.

#define PROBE(name, NIN, NOUT, BODY)                                                              \
  __kernel void name(__global const uint* in, __global uint* out, uint n) {                       \
    const uint i = (uint)get_global_id(0);                                                        \
    if (i >= n) return;                                                                           \
    __global const uint* a = in + (size_t)i * NIN;                                                \
    __global uint* r = out + (size_t)i * NOUT;                                                    \
    BODY                                                                                          \
  }

#define F(k) as_float(a[k])
#define F4(k) ((float4)(F(k), F(k + 1), F(k + 2), F(k + 3)))
#define D(k) as_double(((ulong)a[2 * (k) + 1] << 32) | (ulong)a[2 * (k)])
#define PUT4(v) r[0] = as_uint((v).x); r[1] = as_uint((v).y); r[2] = as_uint((v).z); r[3] = as_uint((v).w);

PROBE(probe_normalize, 4, 4, const float4 v = normalize(F4(0)); PUT4(v))
PROBE(probe_distance, 8, 1, r[0] = as_uint(distance(F4(0), F4(4)));)
PROBE(probe_dot4, 8, 1, r[0] = as_uint(dot(F4(0), F4(4)));)
PROBE(probe_dot2, 4, 1, r[0] = as_uint(dot((float2)(F(0), F(1)), (float2)(F(2), F(3))));)
PROBE(probe_cross, 8, 4, const float4 v = cross(F4(0), F4(4)); PUT4(v))
PROBE(probe_clamp01, 1, 1, r[0] = as_uint(clamp(F(0), 0.0f, 1.0f));)
PROBE(probe_sin, 1, 1, r[0] = as_uint(sin(F(0)));)
PROBE(probe_cos, 1, 1, r[0] = as_uint(cos(F(0)));)
PROBE(probe_fdiv, 2, 1, r[0] = as_uint(F(0) / F(1));)
PROBE(probe_rcp, 1, 1, r[0] = as_uint(1.0f / F(0));)
PROBE(probe_div25, 1, 1, r[0] = as_uint(F(0) / 25.0f);)
PROBE(probe_sqrt, 1, 1, r[0] = as_uint(sqrt(F(0)));)
PROBE(probe_rsqrt, 1, 1, r[0] = as_uint(rsqrt(F(0)));)
PROBE(probe_mad1, 3, 1, r[0] = as_uint(F(0) * F(1) + F(2));)
PROBE(probe_mad2, 4, 1, r[0] = as_uint(F(0) * F(1) + F(2) * F(3));)
PROBE(probe_mad3, 6, 1, r[0] = as_uint(F(0) * F(1) + F(2) * F(3) + F(4) * F(5));)
PROBE(probe_mad1d, 6, 2, const ulong v = as_ulong(D(0) * D(1) + D(2)); r[0] = (uint)v; r[1] = (uint)(v >> 32);)
