/*
 * lenstrace_hip.h -- C ABI of the MI355X-native lens_trace ray-trace backend (liblenstrace-hip.so).
 *
 * This is the drop-in boundary: plain pointers and sizes, POD structs, int status codes, no C++
 * types and no exceptions.  It carries exactly what the reference's renderer plugin does inside
 * Renderer::render() (all citations relative to the reference tree):
 *
 *   reference step                                                         replaced by
 *   ---------------------------------------------------------------------  -------------------------
 *   RendererOpenCL::RendererOpenCL(), device/context/queue                  lt_hip_create
 *     src/opencl/renderer_opencl.cpp:11-24
 *   ~RendererOpenCL()                          :26-33                       lt_hip_destroy
 *   compileKernel(path) + programMap lookup    :35-54, :67-70               lt_hip_program_from_path
 *     (a kernel *source path* selects the program; here its basename
 *      selects one of the five pre-compiled HIP programs)
 *   5 x clCreateBuffer + clEnqueueWriteBuffer  :107-120                     lt_hip_set_scene
 *     (node / ordered-primitive / material / light-container buffers;
 *      uploaded once and cached instead of on every render() call)
 *   the two together, per render() call                                    lt_hip_render_scene
 *   camera buffer upload + kernel args + NDRange launches + wait +          lt_hip_render
 *     blocking read-back into pOutputBuffer    :119-149                     (lt_hip_render_device keeps
 *                                                                            the pixels in HBM)
 *   examples/accumulator frame loop + accumulator.frag running mean         frame_count / accumulate
 *     examples/accumulator/src/main.cpp:296-325, shaders/accumulator.frag   fields of lt_hip_render_desc
 *   printf("Kernel Error: %d") / build log     :3-9, :142-144               lt_hip_last_error
 *
 * Launch semantics are the CUDA backend's (src/cuda/renderer_cuda.cpp:74-88): every pixel of the
 * W x H image is rendered exactly once, whatever W and H are (the OpenCL backend's truncating
 * work-block maths, renderer_opencl.cpp:90, is a launch-decomposition artefact the reference's own
 * CustomBlockSize test declares invisible).
 *
 * Buffer layouts are the reference's, verbatim:
 *   nodes     LinearBVHNode[M] 32 B  include/lens_trace/acceleration_structure_explicit.h:20-32
 *   prims     Primitive[N]     76 B  :34-42 (BVH order)
 *   materials Material[K]      32 B  include/lens_trace/model.h:26-31
 *   lights    LightContainer  260 B  acceleration_structure_explicit.h:44-47
 *   camera    7 x 4 B                src/camera.cpp:14-19 (frameCount uint in the 7th slot)
 *   output    float[H][W][depth], 3 floats written per pixel at (y*W+x)*depth
 */
#ifndef LENSTRACE_HIP_H
#define LENSTRACE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LT_HIP_ABI_VERSION 4

typedef struct lt_hip_context lt_hip_context;

/* status codes (0 = success) */
enum {
  LT_OK = 0,
  LT_ERR_INVALID_ARGUMENT = 1,
  LT_ERR_NO_DEVICE = 2,      /* no usable gfx950 device / HIP runtime failure at create */
  LT_ERR_HIP = 3,            /* a HIP call failed; text in lt_hip_last_error */
  LT_ERR_NO_SCENE = 4,       /* render before set_scene */
  LT_ERR_BAD_SCENE = 5,      /* index out of range, BVH deeper than the reference's 64-entry stack, ... */
  LT_ERR_BUFFER_TOO_SMALL = 6,
  LT_ERR_UNKNOWN_PROGRAM = 7
};

/* the kernel files the reference ships (five renderer programs + the custom_kernel example's), selected by kernelFilePath in RenderProperties* */
enum {
  LT_PROGRAM_BASIC = 0,                  /* resources/kernels/opencl/basic.cl */
  LT_PROGRAM_BASIC_LIGHTING = 1,         /* resources/kernels/opencl/basic_lighting.cl (25 blended samples) */
  LT_PROGRAM_ACCUMULATOR = 2,            /* examples/accumulator/resources/kernels/accumulator.cl */
  LT_PROGRAM_GLOBAL_ILLUMINATION = 3,    /* examples/global_illumination/resources/kernels/global_illumination.cl */
  LT_PROGRAM_GLOBAL_ILLUMINATION_25 = 4, /* resources/kernels/opencl/global_illumination.cl (25 blended samples) */
  LT_PROGRAM_CUSTOM_OPENCL = 5           /* examples/custom_kernel/resources/kernels/custom_opencl.cl (barycentrics as colour) */
};

/* KernelMode of include/lens_trace/structures.h:20-23.  Pixels do not depend on it, except that the
 * lighting programs' linearKernel clamps to [0,1] and their tileKernel does not (accumulator.cl:316-318
 * vs :356-358). */
enum { LT_KERNEL_MODE_LINEAR = 0, LT_KERNEL_MODE_TILE = 1 };

enum {
  LT_RENDER_FLAG_STATS = 1u,    /* count rays / node visits / triangle tests with device atomics (slower) */
  LT_RENDER_FLAG_PIXEL_COUNTERS = 2u,/* diagnostic (implies STATS, needs depth >= 4): instead of the colour, write each
                                        pixel's own {rays, shadow rays, node visits, triangle tests} as 4 floats */
  LT_RENDER_FLAG_DEVICE_LIBM = 4u,   /* accepted and ignored (ABI 2 name of what became LT_RENDER_FLAG_STRICT_MATH) */
  /* Floating-point flavour ("Floating-point model"): what the reference leaves to its OpenCL implementation.
   * DEFAULT (no flag): the reference's kernel files exactly as RendererOpenCL builds them on this GPU -- clBuildProgram with
   *   NULL options (src/opencl/renderer_opencl.cpp:50): `a*b + c` inside one source expression is one fused multiply-add,
   *   float divide / sqrt have the OpenCL default accuracy (v_rcp_f32 / v_sqrt_f32 based), the builtins (dot, cross,
   *   normalize, distance, sin, cos, clamp) are ROCm's OpenCL device library's.  Output is bit-identical to those kernels
   *   (tests/test_gpu_reference_kernels.py, test_gpu_full_size.py, test_gpu_configs.py).
   * LT_RENDER_FLAG_STRICT_MATH: the same kernels built with -ffp-contract=off -cl-fp32-correctly-rounded-divide-sqrt: one IEEE
   *   operation per source operation outside the builtins.  Bit-identical to that build.
   * LT_RENDER_FLAG_PORTABLE_MATH: strict, and the four builtin leaf functions where the device library uses hardware
   *   approximations (rsqrt, sqrt, sinf / cosf, clamp) in correctly rounded forms every IEEE machine reproduces: what the CPU
   *   oracle computes.  Differs from STRICT by <= 1-2 ulp in those functions, which the stochastic programs' random() can
   *   amplify into a flipped ray decision in ~0.03 % of pixels.
   * PORTABLE and STRICT exclude each other. */
  LT_RENDER_FLAG_PORTABLE_MATH = 8u,
  LT_RENDER_FLAG_STRICT_MATH = 16u,
  /* The first accumulator / basic_lighting call of a (scene, image geometry, frames per launch) runs its launch once per
   * shadow-ray walk (4-5 extra launches inside that call, a host-side wait for their times, all of it counted in that call's
   * kernel_ms / kernel_launches) and keeps the fastest.  With this flag a call that has no verdict yet times nothing: it uses
   * the scene's most recent verdict for the program, or any-hit packets.  Pixels do not depend on the walk. */
  LT_RENDER_FLAG_NO_WALK_TIMING = 32u
};

typedef struct lt_hip_render_desc {
  uint32_t struct_size;         /* sizeof(lt_hip_render_desc), for ABI growth */
  int32_t program;              /* LT_PROGRAM_* */
  int32_t kernel_mode;          /* LT_KERNEL_MODE_* */
  uint32_t width, height, depth;/* imageDimensions[3]; depth >= 3 */
  uint8_t camera[28];           /* Camera::getCameraBuffer() */
  /* Progressive rendering (examples/accumulator/src/main.cpp:296-325).  frame_count == 0: one frame with
   * the camera buffer's own frameCount, plain overwrite -- exactly Renderer::render().  frame_count > 0:
   * frames with frameCount = frame_first .. frame_first+frame_count-1; with accumulate != 0 they are folded
   * into the output by accumulator.frag's running mean acc = (c + acc*n)/(n+1), n = accumulate_base,
   * accumulate_base+1, ... (n == 0 replaces); with accumulate == 0 the last frame wins.
   * An accumulating call renders all its frames in one kernel launch (up to LT_FUSED_BYTES of scratch memory,
   * default 16 GiB, per launch) and folds them in frame order: same floats as frame_count calls of one frame,
   * without their per-launch cost -- pass as many frames per call as the application allows. */
  uint32_t frame_first;
  uint32_t frame_count;
  uint32_t accumulate;
  uint32_t accumulate_base;
  /* Image-tile sharding (one process per GPU).  The image is cut into tile_w x tile_h tiles, row-major,
   * edge tiles clipped; this call renders tiles tile_first, tile_first+tile_stride, ... and stores tile k of
   * the call contiguously at float offset k*tile_w*tile_h*depth, row pitch tile_w (pixels of clipped tiles
   * outside the image are not written).  tile_w == 0 means "whole image as one tile", which makes the
   * output layout the reference's (y*W+x)*depth. */
  uint32_t tile_w, tile_h;
  uint32_t tile_first, tile_stride;
  int32_t gi_max_depth;         /* 0 = the reference constant 16 (global_illumination.cl:307) */
  uint32_t flags;               /* LT_RENDER_FLAG_* */
} lt_hip_render_desc;

typedef struct lt_hip_stats {
  uint64_t rays;                /* calls of intersect + intersectIgnorePrimitiveIndex (valid with FLAG_STATS) */
  uint64_t shadow_rays;
  uint64_t node_visits;         /* intersectBounds calls */
  uint64_t tri_tests;           /* intersectTriangle calls */
  uint64_t pixels;              /* pixels rendered by the last call (per frame) */
  uint32_t frames;              /* frames rendered by the last call */
  uint32_t kernel_launches;
  float kernel_ms;              /* HIP-event time over the kernels of the last call, on the call's stream */
  float total_ms;               /* lt_hip_render only: upload + kernels + read-back wall time */
  float render_ms;              /* kernel_ms without the running-mean kernels that follow fused multi-sample launches */
  int32_t shadow_packets;       /* how the last call walked its shadow rays: 1 = any-hit packets, 0 = per lane, 2 = chosen per wavefront,
                                 * 3 = queued and walked by a kernel of their own whose lanes take a new ray when theirs is done
                                 * (accumulator; picked per scene, program, image geometry and frames per launch by timing the
                                 * candidates once; LT_SHADOW_PACKETS=0/1/2/3 forces), -1 = not timed yet */
  uint32_t scene_uploads;       /* lt_hip_set_scene calls of this context that uploaded ... */
  uint32_t scene_reused;        /* ... and those that found the resident scene's content unchanged (full hash) and kept it */
  int32_t own_tree_height;      /* height of the backend's own hierarchy over the scene's leaves (built at lt_hip_set_scene, walked by
                                 * every finite ray of the non-counting kernels; LT_RETREE=0 keeps the caller's splits), -1 = none: every walk uses the caller's tree */
  float own_tree_ms;            /* time of its preparation inside lt_hip_set_scene (device or host) */
} lt_hip_stats;

int lt_hip_abi_version(void);

/* device_index: HIP ordinal (one context per GPU, one process per GPU under torch.distributed). */
int lt_hip_create(int device_index, lt_hip_context** out_ctx);
int lt_hip_destroy(lt_hip_context* ctx);

/* Text of the last error on ctx (or of the last failed lt_hip_create when ctx == NULL). Never NULL. */
const char* lt_hip_last_error(const lt_hip_context* ctx);

/* Maps RenderProperties*::kernelFilePath to LT_PROGRAM_* by basename ("…/accumulator.cl" -> ACCUMULATOR).
 * "global_illumination" resolves to the 25-sample program when the path contains "resources/kernels/opencl/"
 * and does not contain "examples/", as in the reference tree. */
int lt_hip_program_from_path(const char* kernel_file_path, int* out_program);

/* program ids >= LT_PROGRAM_USER_BASE are user programs of one context, handed out by lt_hip_resolve_program */
#define LT_PROGRAM_USER_BASE 1000

/* The reference's "kernelFilePath names a source file that is compiled at first use and cached by path"
 * (renderer_opencl.cpp:35-54, :67-70): a path whose basename is a built-in program resolves like
 * lt_hip_program_from_path; any other path ending in ".hip" is read as a USER PROGRAM -- a HIP source file defining
 *     template <class CFG> __device__ lt::V3 lt::user_shade(const SceneDev&, const Ray& cameraRay, float filmX, float filmY,
 *                                                            uint32_t frameCount, Stack<CFG::kDeep>&, Counters&);
 * (the shade step; traversal, camera rays, framebuffer and scheduling are the built-in ones, lens_trace_amd/csrc/lt_kernel.hpp)
 * -- compiled for gfx950 with hipRTC (-O3 -ffp-contract=off), cached by path for the life of the context.  Compile errors
 * are reported through lt_hip_last_error (LT_ERR_UNKNOWN_PROGRAM). */
int lt_hip_resolve_program(lt_hip_context* ctx, const char* kernel_file_path, int* out_program);

/* Uploads (host pointers) and validates the four scene buffers; keeps them resident until the next
 * set_scene / destroy.  A call whose four buffers have the sizes and the content (a hash of every byte) of the resident
 * scene returns at once and keeps it: callers may pass their scene on every render, as the reference does
 * (renderer_opencl.cpp:107-120), and in-place edits are honoured.
 * Derived at upload: the traversal-side triangle array (48-byte stride: A, B-A, C-A) and -- when every node's box encloses
 * its children's, which the reference's own builder guarantees -- the backend's OWN hierarchy over the caller's leaves
 * (binned surface-area heuristic, built by kernels -- lens_trace_amd/csrc/lt_prep.hip: ~6.5 ms for the whole call on a million
 * triangles -- or, for small or unusual buffers, by host threads: lt_retree.hpp), the 64-byte records of its packet
 * walks, the 4-wide groups of quantised boxes and the leaf records of its per-lane walks and the reference's leaf order per
 * direction-sign octant.  The caller's LinearBVHNode array stays resident and is
 * what the counting kernels (LT_RENDER_FLAG_STATS / _PIXEL_COUNTERS), rays with a non-finite component and scenes whose
 * boxes do not nest walk, in the reference's order.  Pixels do not depend on which hierarchy a ray walked
 * (lens_trace_amd/csrc/lt_retree.hpp).  LT_RETREE=0 keeps the caller's splits. */
int lt_hip_set_scene(lt_hip_context* ctx, const void* nodes, uint64_t node_bytes, const void* prims,
                     uint64_t prim_bytes, const void* materials, uint64_t material_bytes, const void* lights,
                     uint64_t light_bytes);

/* Number of floats the output of `desc` needs (whole image: W*H*depth; tiled: tiles_of_call*tile_w*tile_h*depth). */
int lt_hip_output_floats(const lt_hip_render_desc* desc, uint64_t* out_floats);

/* Reference semantics: synchronous, fills caller-owned HOST memory (pOutputBuffer). */
int lt_hip_render(lt_hip_context* ctx, const lt_hip_render_desc* desc, float* out_host, uint64_t out_bytes);

/* lt_hip_set_scene followed by lt_hip_render, as one call -- what a plugin's render() does with a caller that hands over its
 * scene every time (renderer_opencl.cpp:107-120).  Same results and same statuses as the two calls; when the four buffers have
 * the resident scene's sizes the frame is rendered while the host hashes them, and rendered again only if they turn out to have
 * changed -- so that an unchanged scene costs no hashing time on top of the frame.  After a call that found the scene changed
 * (an animation) the next call hashes first: a millisecond in front of the frame instead of a frame rendered for nothing. */
int lt_hip_render_scene(lt_hip_context* ctx, const void* nodes, uint64_t node_bytes, const void* prims, uint64_t prim_bytes,
                        const void* materials, uint64_t material_bytes, const void* lights, uint64_t light_bytes,
                        const lt_hip_render_desc* desc, float* out_host, uint64_t out_bytes);

/* Same, but the pixels stay in HBM: out_device is device memory of the context's GPU, the work is enqueued
 * on hip_stream (a hipStream_t, NULL = default stream) and NOT waited for.
 * Streams: a render's scratch is the context's -- work counters, sample images and the camera hits that accumulator keeps from one
 * call to the next for as long as scene, camera, image and tile set stay what they were (lt_hip_camera_hit_passes).  A render
 * enqueued on another stream than the render before it on this context waits (hipStreamWaitEvent, on the device; the host does not
 * wait) for that render's last launch before its own first: a call that reuses the hits starts after the launch that wrote them, a
 * call that overwrites them after their last reader.  Renders on one stream are ordered by the stream, and no wait is added.  The
 * output buffers are the caller's to order. */
int lt_hip_render_device(lt_hip_context* ctx, const lt_hip_render_desc* desc, float* out_device,
                         uint64_t out_bytes, void* hip_stream);

/* Scatters a gathered stack of per-rank tile buffers (rank r holds tiles r, r+n_ranks, ...) into the
 * reference's row-major image.  All pointers are device memory; runs on hip_stream.  The image: at most 2^31 - 1 pixels, as for
 * the render calls (LT_ERR_INVALID_ARGUMENT, "image too large"). */
int lt_hip_untile(lt_hip_context* ctx, const float* gathered, uint64_t floats_per_rank, uint32_t n_ranks,
                  uint32_t width, uint32_t height, uint32_t depth, uint32_t tile_w, uint32_t tile_h,
                  float* image_out, void* hip_stream);

int lt_hip_synchronize(lt_hip_context* ctx, void* hip_stream);

/* Host only, no context, no GPU: the hierarchy lt_hip_set_scene would build over the leaves of `nodes` (LinearBVHNode array,
 * node_bytes = 32 * count), written to out_nodes (capacity out_bytes; 32 bytes x (2 x leaves - 1)) in the caller's own layout
 * and pre-order numbering, and, when rank8 != NULL, the reference's leaf order (8 uint32 per primitive, n_prims primitives:
 * position of the primitive's leaf in the reference's depth-first order for each direction-sign octant).  Returns the
 * hierarchy's height, or -1 when the scene gets none (boxes that do not nest, fewer than two leaves, bounds >= 2^40).
 * height_slack: levels allowed above ceil(log2 leaves) (lt_hip_set_scene uses 2); < 0 copies the caller's splits. */
int lt_hip_own_hierarchy(const void* nodes, uint64_t node_bytes, int height_slack, void* out_nodes, uint64_t out_bytes,
                         uint32_t* rank8, uint32_t n_prims);

/* Host only, no context, no GPU: what lt_hip_set_scene makes of that hierarchy (own_nodes: the array lt_hip_own_hierarchy wrote)
 * for its per-lane walks -- the tree collapsed into 4-wide groups, numbered depth first.  out_slots receives four 16-byte child
 * slots per group: the child's box on a 16-bit grid over the scene's bounds, rounded outwards, as six uint16 (lo.x lo.y lo.z hi.x
 * hi.y hi.z), then one uint32 link: the child's own group, or 0x80000000 | (groups + primitive offset) for a leaf (the index of its
 * 64-byte record behind the groups); an empty slot holds lo = 65535, hi = 0 and the link 0x80000000 | (groups + n_prims).
 * origin_step receives the grid: origin xyz, step xyz (bound = origin + q * step); *out_groups the number of groups (at most
 * leaves - 1: size out_slots for that).  Returns the height of the group tree, or -1 (bad arguments, two leaves on one
 * primitive, a bound off the grid).  The same arithmetic runs on the GPU at upload (lens_trace_amd/csrc/lt_own16.hpp). */
int lt_hip_own_wide(const void* own_nodes, uint64_t node_bytes, uint32_t n_prims, float* origin_step, void* out_slots, uint64_t out_bytes,
                    uint32_t* out_groups);

/* Diagnostics: copies one of the structures lt_hip_set_scene derived for the resident scene back to the host (tests hold the
 * device-side preparation, lens_trace_amd/csrc/lt_prep.hip, against the host-side one, lt_retree.hpp, with it).
 * what: 0 = the own tree (32-byte nodes, pre-order), 1 = the leaf order table (8 x uint32 per primitive), 2 = the per-lane
 * walks' array (64-byte grid header, then 64-byte records: groups, leaf records by primitive offset, the sentinel),
 * 3 = four uint32: own-tree height, group-tree height, groups, 1 if the device prepared the scene (0: the host),
 * 4 = the packet walks' records (64 bytes per node of the own tree: an interior node's two children -- box pushed outwards,
 * reference with bit 31 set for a leaf, 0.0f -- or a leaf's triangle A, B - A, C - A, its box bit for bit, its primitive offset),
 * 5 = the traversal triangles (48 bytes per primitive: A, B - A, C - A, three zero floats).
 * out == NULL: only *out_bytes (the size) is set.  LT_ERR_NO_SCENE without a scene; *out_bytes = 0 for kinds 0, 1, 2 and 4 when
 * the scene has no such structure (it then walks the caller's tree); kinds 3 and 5 are always there.  In kind 2 the leaf records of
 * primitive offsets that no leaf names are written by nobody. */
int lt_hip_read_scene_structure(lt_hip_context* ctx, int what, void* out, uint64_t capacity, uint64_t* out_bytes);

/* The scene from bare triangles: the four buffers lt_hip_set_scene wants -- the pre-order LinearBVHNode tree, the ordered 76-byte
 * primitives, the light container; the materials pass through -- built by the CANONICAL MEDIAN BUILD, the rule of the reference's
 * AccelerationStructureExplicit (median split, ACCELERATION_STRUCTURE_TYPE_BVH) with the two places it leaves to the
 * implementation fixed: the order of triangles whose centres coincide, and the sign of a zero bound.
 *
 * Per triangle i (its index in the input), for each axis:
 *   lo, hi   the IEEE 754-2019 minimum / maximum of the three vertices (minimum(-0, +0) = -0, maximum(-0, +0) = +0);
 *   c        0.5f * lo + 0.5f * hi: two rounded products, one rounded sum, never a fused multiply-add.
 * A range of count >= 2 triangles (the root's range is all of them), for node number `node`:
 *   d[a]     max c[a] - min c[a] over the range, one rounded subtraction;
 *   dim      (d[0] > d[1] && d[0] > d[2]) ? 0 : (d[1] > d[2] ? 1 : 2);
 *   order    the range by (c[dim], i): floats compared by value (-0 == +0), equal values by the lower input index.  The first
 *            floor(count / 2) go left, the others right.  (d[dim] == 0 is no special case: the range then splits by input index.)
 *   node     axis = dim, primitiveCount = 0, pad = 0, secondChildOffset = node + 2 * floor(count / 2); the left child is node + 1.
 * A range of one triangle is a leaf: primitivesOffset = its position in the ordered buffer (leaves are numbered left to right),
 * primitiveCount = 1, axis = 0, pad = 0.  So the shape -- node numbers, offsets, every node's range, the height ceil(log2 n) --
 * depends on n alone; the data decide the permutation, the axes and the boxes.
 * Boxes: a leaf's is its triangle's lo / hi, an interior node's the IEEE minimum / maximum of its children's: no bound depends on
 * the order it was folded in.
 * Primitives: the input permuted into leaf order, in the 76-byte layout (positions, normals, materialIndex; material_indices ==
 * NULL: every index 0).  Lights: the first 64 positions of the ordered buffer, ascending, whose material has any emission
 * component > 0; count is capped at 64 and the unused slots are 0.  Materials: unchanged.
 * Whenever no two triangles share their centre on all three axes this is the output of the reference's builder with the median
 * rule: every field byte for byte, the box floats by value (a zero bound may differ in sign).
 *
 * Errors, in order: LT_ERR_INVALID_ARGUMENT for a null ctx / desc, struct_size too small, flags != 0, n == 0, null positions,
 * normals or materials, material_bytes == 0 (device form: a pointer that is not 4-byte aligned); LT_ERR_BAD_SCENE for
 * material_bytes that is no multiple of 32 and for lt_hip_set_scene's size limits (4 GiB of nodes, 2 GiB of traversal triangles);
 * then, from the data, LT_ERR_BAD_SCENE for a vertex coordinate that is NaN or infinite ("non-finite vertex position") and for a
 * materialIndex outside [0, material_bytes / 32).  A failed call leaves the resident scene as it was. */
typedef struct lt_hip_triangles_desc {
  uint32_t struct_size;             /* >= sizeof(lt_hip_triangles_desc) */
  uint32_t flags;                   /* 0 */
  uint64_t n;                       /* triangles */
  const float* positions;           /* 9 floats per triangle: A, B, C */
  const float* normals;             /* 9 floats per triangle: the normals at A, B, C */
  const int32_t* material_indices;  /* one per triangle, or NULL: all 0 */
  const void* materials;            /* 32-byte Material records */
  uint64_t material_bytes;
} lt_hip_triangles_desc;            /* 56 B */

/* Host pointers, synchronous: the arrays are uploaded as they are and the four buffers built by kernels (lens_trace_amd/csrc/
 * lt_build.hip), for every n >= 1; what lt_hip_set_scene derives from its buffers is then derived from these, by the same rule
 * (on the device from 8192 nodes on, LT_DEVICE_BUILD=0 / 1 forces; a tree the device preparation declines -- a bound of 2^40 or
 * more -- and small scenes go through a copy on the host).  The scene counts as uploaded (lt_hip_stats::scene_uploads); it has no
 * host image, so a later lt_hip_set_scene / lt_hip_render_scene never finds its buffers "unchanged", whatever their sizes. */
int lt_hip_set_triangles(lt_hip_context* ctx, const lt_hip_triangles_desc* desc);
/* Device pointers of the context's GPU (every pointer of desc).  Waits for the earlier work of hip_stream (a hipStream_t, NULL =
 * default stream) and returns when the scene is resident: the caller's arrays are free to reuse, the context keeps its own
 * 76-byte copy. */
int lt_hip_set_triangles_device(lt_hip_context* ctx, const lt_hip_triangles_desc* desc, void* hip_stream);
/* The same rule in plain C++: host only, no context, no GPU (errors through lt_hip_last_error(NULL)).  nodes receives 32 (2 n - 1)
 * bytes, prims 76 n bytes, lights 260 bytes; LT_ERR_BUFFER_TOO_SMALL when node_bytes or prim_bytes is less. */
int lt_hip_build_scene_host(const lt_hip_triangles_desc* desc, void* nodes, uint64_t node_bytes, void* prims, uint64_t prim_bytes, void* lights);
/* Copies one of the four resident scene buffers back to the host, whichever call made them resident: which 0 = nodes, 1 =
 * primitives, 2 = materials, 3 = lights.  out == NULL: only *out_bytes (the size) is set.  LT_ERR_NO_SCENE without a scene,
 * LT_ERR_BUFFER_TOO_SMALL when capacity is less than the size. */
int lt_hip_read_scene_buffer(lt_hip_context* ctx, int which, void* out, uint64_t capacity, uint64_t* out_bytes);

/* Ray queries over the resident scene (the scene of the last lt_hip_set_scene).  Each ray is traced as the reference traces
 * one of its own -- `intersect`, or `intersectIgnorePrimitiveIndex` when ignore >= 0 (accumulator.cl:132-217) -- from the
 * payload {t = tmax, primitiveIndex = hitType = 0}, over the caller's LinearBVHNode tree in the reference's order, with the
 * intersectTriangle epsilon of the kernel file `program` names (basic.cl:77-117 and custom_opencl: 1e-7f compared in float;
 * basic_lighting.cl:4: 1e-7 in double; the three others: 1e-4 in double).  Kept as the reference has them: no t > 0 test, no
 * tmin, `t < tmax` with tmax as given (0, negative, inf and NaN included).  The kernel sets origin.w = 1, direction.w = +0.
 * The walk may follow the backend's own hierarchy: results are the same bit for bit (equal t from two triangles: the
 * reference's first leaf wins).  lens_trace_amd/csrc/lt_query.hip.
 * Streams: the ray, point, box and triangle queries (lt_hip_trace_rays, lt_hip_trace_hits, lt_hip_trace_surface,
 * lt_hip_nearest_points, lt_hip_nearest_k, lt_hip_nearest_list, lt_hip_overlap_boxes, lt_hip_overlap_tris,
 * lt_hip_overlap_boxes_list, lt_hip_overlap_tris_list, host and _device forms) share the context's work counters, so calls of these entry
 * points are ordered among themselves on any streams (each waits for the one enqueued before it). */
typedef struct lt_hip_ray { float origin[3]; float tmax; float direction[3]; int32_t ignore; } lt_hip_ray;   /* 32 B, ignore -1 = none */
typedef struct lt_hip_hit { float t; int32_t prim; float u, v; } lt_hip_hit;   /* 16 B; a miss: prim = -1, t = tmax, u = v = 0 */

/* LT_TRACE_CLOSEST writes one lt_hip_hit per ray; LT_TRACE_ANY one uint32 per ray: 1 when the closest-hit query of the same
 * ray would report prim >= 0, else 0 (the walk may stop at the first accepted triangle). */
enum { LT_TRACE_CLOSEST = 0, LT_TRACE_ANY = 1 };
/* flags: LT_RENDER_FLAG_STRICT_MATH or LT_RENDER_FLAG_PORTABLE_MATH (the render path's meaning; default: as shipped), and */
#define LT_TRACE_FLAG_COHERENT 0x100u   /* caller promises: runs of 64 consecutive rays are coherent (walked as packets) */

typedef struct lt_hip_trace_desc {
  uint32_t struct_size;         /* >= sizeof(lt_hip_trace_desc) */
  int32_t program;              /* a built-in LT_PROGRAM_* (selects the epsilon) */
  int32_t kind;                 /* LT_TRACE_CLOSEST / LT_TRACE_ANY */
  uint32_t flags;
} lt_hip_trace_desc;

/* Host memory, synchronous.  LT_ERR_INVALID_ARGUMENT: null ctx / desc, a null pointer with n > 0, an unknown kind, n >= 2^32, a
 * user program, STRICT with PORTABLE, any other flag, struct_size too small (and, device entry point, pointers that are not
 * 16-byte aligned); with LT_TRACE_FLAG_COHERENT also n > 2^32 - 64 (one workgroup per 64 rays: from 2^32 - 63 rays on that is
 * 2^32 work-items, more than a launch can hold; lt_hip_trace_surface likewise); LT_ERR_NO_SCENE; LT_ERR_BUFFER_TOO_SMALL when
 * out_bytes < n records.  A failed call writes nothing to out; n == 0 launches nothing.  lt_hip_get_stats then reports rays = n
 * (closest) or shadow_rays = n (any), kernel_launches and kernel_ms. */
int lt_hip_trace_rays(lt_hip_context* ctx, const lt_hip_trace_desc* desc, const lt_hip_ray* rays, uint64_t n,
                      void* out, uint64_t out_bytes);
/* Device memory of the context's GPU, enqueued on hip_stream (a hipStream_t, NULL = default stream), not waited for. */
int lt_hip_trace_rays_device(lt_hip_context* ctx, const lt_hip_trace_desc* desc, const lt_hip_ray* rays, uint64_t n,
                             void* out, uint64_t out_bytes, void* hip_stream);

/* Multi-hit ray queries: what lies BEHIND the first surface, in one walk -- transparency, lens stacks, thickness and
 * penetration counts, inside / outside by crossing parity.  (A second lt_hip_trace_rays from the hit point would need an offset
 * the reference's rules do not have, and `ignore` names one primitive only.)
 *
 * The HIT SEQUENCE of a ray {origin, tmax, direction, ignore} under an epsilon program is defined by peeling.  Hit 0 is what the
 * reference's `intersect` (`intersectIgnorePrimitiveIndex` when ignore >= 0) returns from the payload {t = tmax, primitiveIndex =
 * hitType = 0}: what lt_hip_trace_rays / LT_TRACE_CLOSEST reports.  Hit j is what the same call returns on the same scene after
 * the primitives of hits 0 .. j-1 have been made degenerate (B = C = A: intersectTriangle rejects such a primitive for every ray,
 * and the node boxes stay as they are).  The sequence ends at the first miss.  Equivalently: it holds, once each, every primitive
 * whose leaf the reference's box tests reach and which intersectTriangle accepts with t < tmax, in ascending t by the float `<`;
 * primitives of bit-equal t (-0 == +0) in the reference's traversal order for that ray.  Everything else is lt_hip_trace_rays':
 * no t > 0 test, no tmin, tmax as given (0, negative, inf, NaN), origin.w = 1, direction.w = +0, the `ignore` leaf is never
 * entered, a leaf with primitiveCount > 1 tests its one primitive once.  (The reference's builder never makes two leaves that name
 * one primitive.  A scene that has such leaves gets no own hierarchy, and there a primitive may appear once per leaf.)
 *
 * LT_TRACE_FIRST_K writes the first max_hits entries of the sequence as max_hits consecutive lt_hip_hit records per ray, ray-major
 * (record i * max_hits + j is hit j of ray i); unused slots hold the miss record {t = tmax, prim = -1, u = v = 0}.
 * LT_TRACE_COUNT writes one uint32 per ray: the length of the whole sequence.
 * flags: LT_RENDER_FLAG_STRICT_MATH or LT_RENDER_FLAG_PORTABLE_MATH, with the render path's meaning.  LT_TRACE_FLAG_COHERENT is
 * accepted and has no effect on these kinds: there is no multi-hit packet walk, every ray walks per lane (lens_trace_amd/csrc/
 * lt_query.hip, lt_query_hits_kernel). */
#define LT_TRACE_MAX_HITS 8
enum { LT_TRACE_FIRST_K = 0, LT_TRACE_COUNT = 1 };   /* kinds of lt_hip_trace_hits only (not lt_hip_trace_desc::kind) */

typedef struct lt_hip_multihit_desc {
  uint32_t struct_size;         /* >= sizeof(lt_hip_multihit_desc) */
  int32_t program;              /* a built-in LT_PROGRAM_* (selects the epsilon) */
  int32_t kind;                 /* LT_TRACE_FIRST_K / LT_TRACE_COUNT */
  uint32_t flags;
  uint32_t max_hits;            /* FIRST_K: 1 .. LT_TRACE_MAX_HITS; COUNT: 0 */
  uint32_t reserved;            /* 0 */
} lt_hip_multihit_desc;         /* 24 B */

/* Host memory, synchronous.  Errors as lt_hip_trace_rays (null ctx / desc, a null pointer with n > 0, an unknown kind, n >= 2^32,
 * a user program, STRICT with PORTABLE, any other flag, struct_size too small; device entry point: pointers that are not 16-byte
 * aligned), and LT_ERR_INVALID_ARGUMENT for max_hits outside 1 .. LT_TRACE_MAX_HITS (FIRST_K), max_hits != 0 (COUNT) or
 * reserved != 0; LT_ERR_UNKNOWN_PROGRAM for a program id that is neither; LT_ERR_NO_SCENE; LT_ERR_BUFFER_TOO_SMALL when out_bytes < n * max_hits * 16 (FIRST_K) or n * 4 (COUNT).  A failed
 * call writes nothing to out; n == 0 launches nothing.  lt_hip_get_stats then reports rays = n, kernel_launches and kernel_ms. */
int lt_hip_trace_hits(lt_hip_context* ctx, const lt_hip_multihit_desc* desc, const lt_hip_ray* rays, uint64_t n,
                      void* out, uint64_t out_bytes);
/* Device memory of the context's GPU, enqueued on hip_stream (a hipStream_t, NULL = default stream), not waited for. */
int lt_hip_trace_hits_device(lt_hip_context* ctx, const lt_hip_multihit_desc* desc, const lt_hip_ray* rays, uint64_t n,
                             void* out, uint64_t out_bytes, void* hip_stream);

/* Hit lists: the WHOLE hit sequence of every ray, as CSR -- every surface of a transparency or lens stack, every crossing for
 * thickness, penetration depth and parity, where LT_TRACE_FIRST_K stops at eight and LT_TRACE_COUNT only says that there are
 * more.  The hit sequence is lt_hip_trace_hits', word for word, without the limit: the peeling definition above, t ascending by the
 * float `<`, bit-equal t (-0 == +0) in the reference's traversal order for that ray, no t > 0 test, tmax as given, the `ignore`
 * leaf never entered; in a scene that gets no own hierarchy (boxes that do not nest, a primitive named by two leaves) it is what
 * the walk in the reference's order reports, once per leaf, equal t in traversal order.
 *   offsets   n + 1 uint64: offsets[i] is the sum of the sequence lengths of rays 0 .. i-1 (an exclusive scan: offsets[0] = 0,
 *             offsets[n] the total).
 *   items     offsets[n] lt_hip_hit records of 16 bytes, {t, prim, u, v}: items[offsets[i] .. offsets[i + 1]) is the whole
 *             sequence of ray i, nearest first.  Every record feeds lt_hip_surface_at as it is.  A ray that hits nothing has an
 *             empty segment: there are no miss records.
 * So the differences of offsets are LT_TRACE_COUNT's words, and the first min(8, length) records of a segment are
 * LT_TRACE_FIRST_K's real records at max_hits = 8, bit for bit in all four fields, in every math flavour.
 * program: a built-in LT_PROGRAM_* (it selects the triangle epsilon), as in lt_hip_multihit_desc.
 * flags: LT_RENDER_FLAG_STRICT_MATH or LT_RENDER_FLAG_PORTABLE_MATH, with the render path's meaning; LT_TRACE_FLAG_COHERENT is
 * accepted and has no effect (there is no multi-hit packet walk); LT_TRACE_LIST_FLAG_FILL_ONLY.  reserved must be 0.
 * Sizing, items that are too small, FILL_ONLY, n == 0 and the statistics are lt_hip_overlap_boxes_list's (below) with 4 bytes per
 * item replaced by 16: items == NULL with items_bytes == 0 writes the offsets only; with items_bytes < 16 offsets[n] nothing is
 * written to items, offsets is written in full, the host-memory form returns LT_ERR_BUFFER_TOO_SMALL and the device form LT_OK;
 * with FILL_ONLY offsets is input and, whatever it holds, ray i writes only into items[offsets[i] .. min(offsets[i + 1],
 * items_bytes / 16)), a length that would be negative being 0; the device entry point takes pointers that are 16-byte aligned;
 * lt_hip_get_stats reports rays = n, kernel_ms and 4 / 2 / 6 kernels launched (one fewer with a fill in a scene without an own
 * hierarchy: nothing is left to order there).
 * Errors, in order: LT_ERR_INVALID_ARGUMENT for a null ctx / desc, struct_size too small, a user program (LT_ERR_UNKNOWN_PROGRAM
 * for an id that is neither), any other flag, STRICT with PORTABLE, reserved != 0, n >= 2^32, null rays or offsets with n > 0,
 * items == NULL with items_bytes != 0, FILL_ONLY with items == NULL (device entry point: pointers that are not 16-byte aligned);
 * LT_ERR_NO_SCENE; LT_ERR_BUFFER_TOO_SMALL when offsets_bytes < 8 (n + 1).  Such a call writes nothing.
 * Cost: the count is LT_TRACE_COUNT's walk, the fill that walk again.  The segments of the rays the backend's own hierarchy takes
 * are then sorted by one wavefront each, up to 1024 records in LDS and longer ones in place in device memory.  A ray that walks
 * in the reference's order (a scene without an own hierarchy, a non-finite ray, magnitudes beyond the own walks') keeps its
 * segment sorted while it fills it, which is quadratic in the segment's length.  Batches whose items pass 4 GiB are untested.
 * There is no _host form: the CPU definition of this family is the peeling itself (tests/multihit.py runs it on the oracle).
 * (lens_trace_amd/csrc/lt_query.hip, lt_overlist.hip) */
#define LT_TRACE_LIST_FLAG_FILL_ONLY 0x200u
typedef struct lt_hip_hits_list_desc {
  uint32_t struct_size;         /* >= sizeof(lt_hip_hits_list_desc) */
  int32_t program;              /* a built-in LT_PROGRAM_* (selects the epsilon) */
  uint32_t flags;
  uint32_t reserved;            /* 0 */
} lt_hip_hits_list_desc;        /* 16 B */

int lt_hip_trace_hits_list(lt_hip_context* ctx, const lt_hip_hits_list_desc* desc, const lt_hip_ray* rays, uint64_t n,
                           uint64_t* offsets, uint64_t offsets_bytes, lt_hip_hit* items, uint64_t items_bytes);
/* Device memory of the context's GPU, enqueued on hip_stream (a hipStream_t, NULL = default stream), not waited for. */
int lt_hip_trace_hits_list_device(lt_hip_context* ctx, const lt_hip_hits_list_desc* desc, const lt_hip_ray* rays, uint64_t n,
                                  uint64_t* offsets, uint64_t offsets_bytes, lt_hip_hit* items, uint64_t items_bytes, void* hip_stream);

/* Shading of caller-supplied rays: a picture through any camera model (pitched, orthographic, fisheye, a calibrated lens, a light
 * probe, a tensor of rays).  For each ray the result is the colour the named program's `shade` returns for it -- what linearKernel /
 * tileKernel would have stored had this ray been a pixel's camera ray at film position (film_x, film_y) and frame frameCount:
 * random() is keyed by the film position and the frame, so two rays with one film position draw the same light samples.
 *   rgb   frames frameCount = frame_first + f, f = 0 .. frame_count - 1, each with linearKernel's [0, 1] clamp of the lighting
 *         programs when kernel_mode == LT_KERNEL_MODE_LINEAR, folded in frame order by accumulator.frag's running mean from n = 0:
 *         what lt_hip_render with accumulate = 1, accumulate_base = 0 leaves in a pixel.  frame_count = 1: the frame itself.
 *   prim  the primitive the ray itself hit, before any lens, or -1 on a miss.
 * The ray's w components are the reference camera's: origin.w = 2 (cameraPosition.w + film.w), direction.w = +0 (aperture.w -
 * film.w).  The camera payload starts at t = FLT_MAX and ignores nothing.
 * Programs: LT_PROGRAM_BASIC (with the lens chain), LT_PROGRAM_BASIC_LIGHTING (25 blended samples per frame), LT_PROGRAM_ACCUMULATOR
 * and LT_PROGRAM_CUSTOM_OPENCL.  The two global-illumination programs and user programs are refused with LT_ERR_INVALID_ARGUMENT:
 * the global-illumination programs have an entry point of their own, lt_hip_shade_paths (below).
 * flags: LT_RENDER_FLAG_STRICT_MATH or LT_RENDER_FLAG_PORTABLE_MATH, with the render path's meaning.  LT_TRACE_FLAG_COHERENT is
 * accepted and has no effect: there is no packet path, every ray walks per lane (lens_trace_amd/csrc/lt_shade.hip). */
typedef struct lt_hip_shade_ray { float origin[3]; float film_x; float direction[3]; float film_y; } lt_hip_shade_ray;   /* 32 B */
typedef struct lt_hip_shade { float rgb[3]; int32_t prim; } lt_hip_shade;                                                /* 16 B */

typedef struct lt_hip_shade_desc {
  uint32_t struct_size;         /* >= sizeof(lt_hip_shade_desc) */
  int32_t program;              /* LT_PROGRAM_BASIC, _BASIC_LIGHTING, _ACCUMULATOR or _CUSTOM_OPENCL */
  int32_t kernel_mode;          /* LT_KERNEL_MODE_LINEAR / LT_KERNEL_MODE_TILE */
  uint32_t flags;
  uint32_t frame_first;
  uint32_t frame_count;         /* >= 1 */
} lt_hip_shade_desc;            /* 24 B */

/* Host memory, synchronous.  LT_ERR_INVALID_ARGUMENT: null ctx / desc, a null pointer with n > 0, n >= 2^32, struct_size too small,
 * STRICT with PORTABLE, any other flag, an unknown kernel_mode, frame_count == 0, a global-illumination or user program (and,
 * device entry point, pointers that are not 16-byte aligned); LT_ERR_UNKNOWN_PROGRAM for an id that is no program;
 * LT_ERR_NO_SCENE; LT_ERR_BUFFER_TOO_SMALL when out_bytes < 16 n.  A failed call writes nothing to out; n == 0 launches nothing.
 * lt_hip_get_stats then reports rays = n, kernel_launches and kernel_ms. */
int lt_hip_shade_rays(lt_hip_context* ctx, const lt_hip_shade_desc* desc, const lt_hip_shade_ray* rays, uint64_t n,
                      lt_hip_shade* out, uint64_t out_bytes);
/* Device memory of the context's GPU, enqueued on hip_stream (a hipStream_t, NULL = default stream), not waited for. */
int lt_hip_shade_rays_device(lt_hip_context* ctx, const lt_hip_shade_desc* desc, const lt_hip_shade_ray* rays, uint64_t n,
                             lt_hip_shade* out, uint64_t out_bytes, void* hip_stream);

/* The global-illumination programs over caller-supplied rays: an environment probe, a 360-degree panorama, a lens model in front
 * of the path tracer.  Records are lt_hip_shade_rays' own: lt_hip_shade_ray in, lt_hip_shade out.
 *   rgb   what lt_hip_render of the same program leaves in a pixel whose camera ray this is, at film position (film_x, film_y),
 *         with frame_count frames from frame_first, accumulate = 1, accumulate_base = 0 and the same gi_max_depth:
 *         LT_PROGRAM_GLOBAL_ILLUMINATION: frame f is shade(ray, film, sampleIndex = frame_first + f), clamped to [0, 1] when
 *         kernel_mode == LT_KERNEL_MODE_LINEAR; LT_PROGRAM_GLOBAL_ILLUMINATION_25: frame f is the 25 samples sampleIndex =
 *         (frame_first + f) * 32 + k blended in order, c = (1 - a) c + a c_k with a = (25 - k) / 25 (sample 0 replaces), the blend
 *         clamped when linear.  The frames are folded in frame order by accumulator.frag's running mean from n = 0.
 *   prim  the primitive the ray itself hit, or -1 on a miss.
 * The ray's w components are the reference camera's (origin.w = 2, direction.w = +0); the camera payload starts at t = FLT_MAX
 * and ignores nothing.  Each ray's camera walk runs once per call, whatever the frames and samples.
 * flags: LT_RENDER_FLAG_STRICT_MATH or LT_RENDER_FLAG_PORTABLE_MATH, with the render path's meaning.  LT_TRACE_FLAG_COHERENT is
 * accepted and has no effect: every ray walks per lane.
 * Scratch memory: 272 bytes per path slot (ray x frame, x 25 for the 25-sample program) of the wavefront pipeline the programs'
 * renders use, in sets of bounded size -- no result depends on how a call is cut into sets (LT_PATHS_SLOTS forces the bound, for
 * tests and measurements; LT_FUSED_BYTES bounds it as it bounds a render's sets).
 * Streams: the scratch and its control block are the context's, shared with the programs' renders.  Calls of this entry point are
 * ordered among themselves on any streams (each waits for the one enqueued before it).  A call and a global-illumination
 * lt_hip_render_device on two different streams are NOT ordered by the library (renders are ordered among themselves, see
 * lt_hip_render_device, and so are calls of this entry point, but not the one with the other): order them (one stream, an event,
 * lt_hip_synchronize) or use two contexts.  (lens_trace_amd/csrc/lt_paths.hip) */
typedef struct lt_hip_paths_desc {
  uint32_t struct_size;         /* >= sizeof(lt_hip_paths_desc) */
  int32_t program;              /* LT_PROGRAM_GLOBAL_ILLUMINATION or LT_PROGRAM_GLOBAL_ILLUMINATION_25 */
  int32_t kernel_mode;          /* LT_KERNEL_MODE_LINEAR / LT_KERNEL_MODE_TILE */
  uint32_t flags;
  uint32_t frame_first;
  uint32_t frame_count;         /* >= 1 */
  int32_t gi_max_depth;         /* 0 = the reference's 16; 1 .. 64 */
  uint32_t reserved;            /* 0 */
} lt_hip_paths_desc;            /* 32 B */

/* Host memory, synchronous.  Errors in lt_hip_shade_rays' order.  LT_ERR_INVALID_ARGUMENT: null ctx / desc, a null pointer with
 * n > 0, n >= 2^32, struct_size too small, STRICT with PORTABLE, any other flag, an unknown kernel_mode, frame_count == 0,
 * gi_max_depth outside 0 .. 64, reserved != 0, one of the four other built-in programs or a user program (the text names
 * lt_hip_shade_rays) (and, device entry point, pointers that are not 16-byte aligned); LT_ERR_UNKNOWN_PROGRAM for an id that is no
 * program; LT_ERR_NO_SCENE; LT_ERR_BUFFER_TOO_SMALL when out_bytes < 16 n.  A failed call writes nothing to out; n == 0 launches
 * nothing.  lt_hip_get_stats then reports rays = n, kernel_launches and kernel_ms. */
int lt_hip_shade_paths(lt_hip_context* ctx, const lt_hip_paths_desc* desc, const lt_hip_shade_ray* rays, uint64_t n,
                       lt_hip_shade* out, uint64_t out_bytes);
/* Device memory of the context's GPU, enqueued on hip_stream (a hipStream_t, NULL = default stream), not waited for. */
int lt_hip_shade_paths_device(lt_hip_context* ctx, const lt_hip_paths_desc* desc, const lt_hip_shade_ray* rays, uint64_t n,
                              lt_hip_shade* out, uint64_t out_bytes, void* hip_stream);

/* Surface queries: what every `shade` of the reference computes first at a hit (accumulator.cl:243-274) -- the point its next ray
 * starts from, the interpolated vertex normal, the primitive's material, whether the primitive is a light -- for a caller that
 * writes its own integrator, sensor model, lightmap baker or denoiser front end on top of the queries.  Per-pixel feature images
 * (position, normal, ids, depth) are a surface query over the camera's rays.
 *   t, prim, u, v   the lt_hip_hit of the same ray, bit for bit: what lt_hip_trace_rays / LT_TRACE_CLOSEST writes for the same
 *                   ray, desc and scene.
 *   position        A*b.x + B*b.y + C*b.z of the primitive's positionA/B/C with b = ((float)(1.0 - u - v), u, v), b.x evaluated
 *                   in double -- NOT origin + t * direction.  As shipped (no flavour flag) the expression is contracted as the
 *                   reference's build contracts it, fma(C, b.z, fma(A, b.x, B * b.y)); LT_RENDER_FLAG_STRICT_MATH and
 *                   LT_RENDER_FLAG_PORTABLE_MATH round the three products and the two sums separately, (A*b.x + B*b.y) + C*b.z.
 *   normal          the same interpolation of normalA/B/C, not normalised (the reference never normalises it).
 *   material        Primitive::materialIndex.
 *   flags           LT_SURFACE_LIGHT when prim is one of LightContainer.primitives[0 .. count - 1] (accumulator.cl:233-237).
 * A miss has position = normal = +0, material = -1, flags = 0. */
typedef struct lt_hip_surface {
  float t; int32_t prim; float u, v;
  float position[3]; int32_t material;
  float normal[3]; uint32_t flags;
} lt_hip_surface;                       /* 48 B */
#define LT_SURFACE_LIGHT 1u

/* lt_hip_trace_surface: from rays to surface records in one call.  desc is lt_hip_trace_rays' own: kind must be LT_TRACE_CLOSEST
 * (LT_TRACE_ANY: LT_ERR_INVALID_ARGUMENT), program selects the triangle epsilon, flags are STRICT or PORTABLE and
 * LT_TRACE_FLAG_COHERENT (honoured: the packet walk).  Host memory, synchronous.  Errors, their order and the alignment rule of
 * the device entry point are lt_hip_trace_rays'; LT_ERR_BUFFER_TOO_SMALL when out_bytes < 48 n.  A failed call writes nothing to
 * out; n == 0 launches nothing.  lt_hip_get_stats then reports rays = n, kernel_launches and kernel_ms.
 * (lens_trace_amd/csrc/lt_query.hip) */
int lt_hip_trace_surface(lt_hip_context* ctx, const lt_hip_trace_desc* desc, const lt_hip_ray* rays, uint64_t n,
                         lt_hip_surface* out, uint64_t out_bytes);
/* Device memory of the context's GPU, enqueued on hip_stream (a hipStream_t, NULL = default stream), not waited for. */
int lt_hip_trace_surface_device(lt_hip_context* ctx, const lt_hip_trace_desc* desc, const lt_hip_ray* rays, uint64_t n,
                                lt_hip_surface* out, uint64_t out_bytes, void* hip_stream);

/* lt_hip_surface_at: the same record from hit records the caller already has -- above all the K records per ray of
 * lt_hip_trace_hits, so that the surfaces behind the first one get positions and normals.  t, u and v are copied bit for bit.  A
 * record whose prim is not one of the scene's primitives (negative, or >= their number) gives the miss form: t as given,
 * prim = -1, u = v = +0, position = normal = +0, material = -1, flags = 0.  lt_hip_trace_surface equals lt_hip_trace_rays followed
 * by lt_hip_surface_at with the same flavour, byte for byte.
 * flags: LT_RENDER_FLAG_STRICT_MATH or LT_RENDER_FLAG_PORTABLE_MATH only; the flavour decides fused or separate multiply-adds and
 * nothing else.  Host memory, synchronous.  LT_ERR_INVALID_ARGUMENT: null ctx / desc, struct_size too small, STRICT with PORTABLE,
 * any other flag, n >= 2^32, a null pointer with n > 0 (and, device entry point, pointers that are not 16-byte aligned);
 * LT_ERR_NO_SCENE; LT_ERR_BUFFER_TOO_SMALL when out_bytes < 48 n.  A failed call writes nothing to out; n == 0 launches nothing.
 * lt_hip_get_stats then reports kernel_launches = 1 and kernel_ms. */
typedef struct lt_hip_surface_desc {
  uint32_t struct_size;         /* >= sizeof(lt_hip_surface_desc) */
  uint32_t flags;
} lt_hip_surface_desc;          /* 8 B */

int lt_hip_surface_at(lt_hip_context* ctx, const lt_hip_surface_desc* desc, const lt_hip_hit* hits, uint64_t n,
                      lt_hip_surface* out, uint64_t out_bytes);
/* Device memory of the context's GPU, enqueued on hip_stream (a hipStream_t, NULL = default stream), not waited for. */
int lt_hip_surface_at_device(lt_hip_context* ctx, const lt_hip_surface_desc* desc, const lt_hip_hit* hits, uint64_t n,
                             lt_hip_surface* out, uint64_t out_bytes, void* hip_stream);

/* Nearest-point queries: for each point the closest primitive of the resident scene, the squared distance and where on the
 * primitive -- for lightmap bakers, sensor models, clearance and collision checks that would otherwise build a second hierarchy.
 * The result is an lt_hip_hit with t = the squared distance, prim, u, v: lt_hip_surface_at turns it straight into the closest
 * point (position), normal, material and light flag.  A miss has prim = -1, t = max_d2 with the bits given, u = v = +0.
 *
 * Candidates: the leaves of the caller's LinearBVHNode array, each with its one primitive (primitivesOffset), as every ray query
 * enumerates them; a leaf with primitiveCount > 1 contributes that one primitive once.
 * Distance of a point P to a candidate:  d2 = max(tri(P; A, e1, e2), box(P; the leaf's box)),  a NaN tri staying a NaN.
 *   tri   on the traversal triangle as the scene stores it, A, e1 = fl(B - A), e2 = fl(C - A), with ap = P - A: four points of the
 *         triangle are tried in this order and the first of the smallest squared distance (by `<`) is kept -- the closest point
 *         of edge AB, (u, v) = (t, 0) with t = (e1.ap) / (e1.e1); of edge AC, (0, t) with t = (e2.ap) / (e2.e2); of edge BC,
 *         (1 - t, t) with t = ((ap - e1).f) / (f.f), f = e2 - e1; each t held to [0, 1] (t > 0 else 0, then t > 1 gives 1: a NaN
 *         counts as 0), so the vertices are the edges' ends; and the foot of the perpendicular, from e2's part at right angles
 *         to e1, g = e2 - k e1 with k = (e1.e2) / (e1.e1): v = (ap.g) / (g.g), u = (e1.ap) / (e1.e1) - v k, where u >= 0, v >= 0
 *         and u + v <= 1.  The point is A + u e1 + v e2 and the squared distance that of r = (ap - u e1) - v e2 per component.
 *         Dot products and squared lengths are (x x' + y y') + z z'.  Every operation is one IEEE float32 operation rounded once,
 *         in this order: nothing is contracted, `/` is the correctly rounded quotient, subnormals are kept
 *         (lens_trace_amd/csrc/lt_nearest.hpp is the expression sequence; tests/nearest.py restates it in numpy).
 *   box   the squared distance from P to the leaf's own box as the caller gave it: per axis g = max(lo - P, P - hi, +0), then
 *         (g.x g.x + g.y g.y) + g.z g.z.
 * Selection: a candidate is accepted iff d2 < max_d2 by the float `<` -- a NaN d2 or a NaN max_d2 never; 0, -0 and negative
 * max_d2 give a miss, inf accepts every finite d2.  Among the accepted the smallest d2 wins, the lowest primitive offset among
 * equal d2.  A point with a component that is not finite is a miss.  The answer is a function of the scene and the point alone:
 * whichever hierarchy is walked, the bits are these.
 *
 * flags: 0.  Host memory, synchronous.  LT_ERR_INVALID_ARGUMENT: null ctx / desc, struct_size too small, flags != 0, n >= 2^32, a
 * null pointer with n > 0 (and, device entry point, pointers that are not 16-byte aligned); LT_ERR_NO_SCENE;
 * LT_ERR_BUFFER_TOO_SMALL when out_bytes < 16 n.  A failed call writes nothing to out; n == 0 launches nothing.
 * lt_hip_get_stats then reports rays = n, kernel_launches = 1 and kernel_ms.  (lens_trace_amd/csrc/lt_nearest.hip) */
typedef struct lt_hip_point { float p[3]; float max_d2; } lt_hip_point;      /* 16 B */
typedef struct lt_hip_nearest_desc {
  uint32_t struct_size;         /* >= sizeof(lt_hip_nearest_desc) */
  uint32_t flags;               /* 0 */
} lt_hip_nearest_desc;          /* 8 B */

int lt_hip_nearest_points(lt_hip_context* ctx, const lt_hip_nearest_desc* desc, const lt_hip_point* points, uint64_t n,
                          lt_hip_hit* out, uint64_t out_bytes);
/* Device memory of the context's GPU, enqueued on hip_stream (a hipStream_t, NULL = default stream), not waited for. */
int lt_hip_nearest_points_device(lt_hip_context* ctx, const lt_hip_nearest_desc* desc, const lt_hip_point* points, uint64_t n,
                                 lt_hip_hit* out, uint64_t out_bytes, void* hip_stream);
/* The same answers on the host, without a context or a GPU, from the caller's buffers: nodes (LinearBVHNode, 32 bytes each) and
 * prims (Primitive, 76 bytes each).  LT_ERR_INVALID_ARGUMENT (a null or mis-sized buffer, n >= 2^32), LT_ERR_BAD_SCENE (a leaf
 * whose offset lies outside prims), LT_ERR_BUFFER_TOO_SMALL (out_bytes < 16 n); a failed call writes nothing. */
int lt_hip_nearest_points_host(const void* nodes, uint64_t node_bytes, const void* prims, uint64_t prim_bytes,
                               const lt_hip_point* points, uint64_t n, lt_hip_hit* out, uint64_t out_bytes);

/* k-nearest queries: the K closest primitives of each point, or how many lie within its radius -- the contact set of a collision
 * or clearance check, the second and third nearest surfaces at thin walls and inner corners, point-to-mesh registration.
 *
 * The candidate sequence of a point {p, max_d2}: candidates, d2, (u, v) and acceptance (d2 < max_d2 by the float `<`) are exactly
 * those of lt_hip_nearest_points; every accepted candidate appears once; the order is ascending d2 by `<`, ascending primitive
 * offset among equal d2 (`==`), and ascending node index in the caller's array among equal d2 and equal offset (only scenes whose
 * leaves name one primitive twice have such candidates).  A point with a component that is not finite, or with a max_d2 nothing
 * is below (0, -0, negative, NaN), has the empty sequence.  The sequence is a function of the scene and the point alone.
 *   LT_NEAREST_FIRST_K  the first max_k entries as max_k consecutive lt_hip_hit records per point, point-major: record
 *                       i * max_k + j is entry j of point i (t = d2, prim, u, v).  Unused slots hold the miss record: t = max_d2
 *                       with the bits given, prim = -1, u = v = +0.  With max_k = 1 the call is lt_hip_nearest_points byte for
 *                       byte.  Every record feeds lt_hip_surface_at as lt_hip_nearest_points' do.
 *   LT_NEAREST_COUNT    one uint32 per point: the length of the whole sequence, i.e. the number of candidates within the radius.
 *                       max_d2 = inf accepts every finite d2, which makes the call a visit of every leaf for every point: give
 *                       a finite radius.
 *
 * flags: 0.  max_k: 1 .. LT_NEAREST_MAX_K for LT_NEAREST_FIRST_K, 0 for LT_NEAREST_COUNT.  Host memory, synchronous.  Errors in
 * lt_hip_nearest_points' order: LT_ERR_INVALID_ARGUMENT for a null ctx / desc, struct_size too small, flags != 0, an unknown kind,
 * max_k outside its range for the kind, n >= 2^32, a null pointer with n > 0 (and, device entry point, pointers that are not
 * 16-byte aligned); LT_ERR_NO_SCENE; LT_ERR_BUFFER_TOO_SMALL when out_bytes < 16 max_k n (FIRST_K) or 4 n (COUNT).  A failed call
 * writes nothing to out; n == 0 launches nothing.  lt_hip_get_stats then reports rays = n, kernel_launches = 1 and kernel_ms.
 * (lens_trace_amd/csrc/lt_nearest.hip) */
#define LT_NEAREST_FIRST_K 0
#define LT_NEAREST_COUNT   1
#define LT_NEAREST_MAX_K   8
typedef struct lt_hip_nearest_k_desc {
  uint32_t struct_size;         /* >= sizeof(lt_hip_nearest_k_desc) */
  uint32_t flags;               /* 0 */
  int32_t kind;                 /* LT_NEAREST_FIRST_K / LT_NEAREST_COUNT */
  uint32_t max_k;               /* FIRST_K: 1 .. LT_NEAREST_MAX_K; COUNT: 0 */
} lt_hip_nearest_k_desc;        /* 16 B */

int lt_hip_nearest_k(lt_hip_context* ctx, const lt_hip_nearest_k_desc* desc, const lt_hip_point* points, uint64_t n,
                     void* out, uint64_t out_bytes);
/* Device memory of the context's GPU, enqueued on hip_stream (a hipStream_t, NULL = default stream), not waited for. */
int lt_hip_nearest_k_device(lt_hip_context* ctx, const lt_hip_nearest_k_desc* desc, const lt_hip_point* points, uint64_t n,
                            void* out, uint64_t out_bytes, void* hip_stream);
/* The same answers on the host, without a context or a GPU, from the caller's buffers, as lt_hip_nearest_points_host takes them.
 * LT_ERR_INVALID_ARGUMENT (a null desc, struct_size, flags, kind or max_k as above, a null or mis-sized buffer, n >= 2^32),
 * LT_ERR_BAD_SCENE (a leaf whose offset lies outside prims), LT_ERR_BUFFER_TOO_SMALL; a failed call writes nothing. */
int lt_hip_nearest_k_host(const void* nodes, uint64_t node_bytes, const void* prims, uint64_t prim_bytes,
                          const lt_hip_nearest_k_desc* desc, const lt_hip_point* points, uint64_t n, void* out, uint64_t out_bytes);

/* Radius lists: the WHOLE candidate sequence of every point, as CSR -- every primitive within the point's radius where
 * LT_NEAREST_FIRST_K stops at eight: the whole contact set of a clearance check, every surface within a tolerance for
 * registration, the neighbours an irradiance or sample cache gathers over, proximity-based occlusion.  Candidates, d2, (u, v),
 * acceptance (d2 < max_d2 by the float `<`), the empty sequence of a point that takes no walk, and the order are
 * lt_hip_nearest_k's, word for word: d2 ascending, then primitive offset, then node index.
 *   offsets   n + 1 uint64: offsets[i] is the sum of the sequence lengths of points 0 .. i-1 (an exclusive scan: offsets[0] = 0,
 *             offsets[n] the total).
 *   items     offsets[n] lt_hip_hit records of 16 bytes, {t = d2, prim, u, v}: items[offsets[i] .. offsets[i + 1]) is the whole
 *             sequence of point i.  Every record feeds lt_hip_surface_at as it is.  (Two records of one point with equal d2 and
 *             equal offset come from the same arithmetic on the same operands and are bit-identical, so the multiset sorted by
 *             (d2, offset) is the sequence: the third key, the node index, orders records that cannot be told apart.  Accepted
 *             d2 are never NaN.)
 * So the differences of offsets are LT_NEAREST_COUNT's words and the first eight records of a segment LT_NEAREST_FIRST_K's real
 * records, bit for bit.
 * Sizing, items that are too small, LT_NEAREST_LIST_FLAG_FILL_ONLY, the errors and their order, n == 0 and the statistics are
 * lt_hip_overlap_boxes_list's (below) with 4 bytes per item replaced by 16: items == NULL with items_bytes == 0 writes the offsets
 * only; with items_bytes < 16 offsets[n] nothing is written to items, offsets is written in full, the host-memory form returns
 * LT_ERR_BUFFER_TOO_SMALL and the device form LT_OK; with FILL_ONLY offsets is input and, whatever it holds, point i writes only
 * into items[offsets[i] .. min(offsets[i + 1], items_bytes / 16)), a length that would be negative being 0; the device entry
 * point takes pointers that are 16-byte aligned; lt_hip_get_stats reports rays = n and 4 / 2 / 6 kernels launched.
 * Cost: the count is LT_NEAREST_COUNT's walk, the fill that walk again; each segment is then sorted by one wavefront, up to 1024
 * records in LDS and longer ones in place in device memory.  max_d2 = inf accepts every finite d2, which makes the call a visit
 * of every leaf for every point and a segment of every leaf: give a finite radius.
 * (lens_trace_amd/csrc/lt_nearest.hip, lt_overlist.hip) */
#define LT_NEAREST_LIST_FLAG_FILL_ONLY 0x1u
typedef struct lt_hip_nearest_list_desc {
  uint32_t struct_size;         /* >= sizeof(lt_hip_nearest_list_desc) */
  uint32_t flags;               /* 0 / LT_NEAREST_LIST_FLAG_FILL_ONLY */
} lt_hip_nearest_list_desc;     /* 8 B */

int lt_hip_nearest_list(lt_hip_context* ctx, const lt_hip_nearest_list_desc* desc, const lt_hip_point* points, uint64_t n,
                        uint64_t* offsets, uint64_t offsets_bytes, lt_hip_hit* items, uint64_t items_bytes);
/* Device memory of the context's GPU, enqueued on hip_stream (a hipStream_t, NULL = default stream), not waited for. */
int lt_hip_nearest_list_device(lt_hip_context* ctx, const lt_hip_nearest_list_desc* desc, const lt_hip_point* points, uint64_t n,
                               uint64_t* offsets, uint64_t offsets_bytes, lt_hip_hit* items, uint64_t items_bytes, void* hip_stream);
/* The same lists on the host, without a context or a GPU, from the caller's buffers, as lt_hip_nearest_k_host takes them: a scan
 * of the caller's leaves in node order, then a stable sort of each segment by (d2, offset).  Errors as above, with
 * lt_hip_nearest_k_host's for the scene (LT_ERR_BAD_SCENE where the context's entry points have LT_ERR_NO_SCENE). */
int lt_hip_nearest_list_host(const void* nodes, uint64_t node_bytes, const void* prims, uint64_t prim_bytes,
                             const lt_hip_nearest_list_desc* desc, const lt_hip_point* points, uint64_t n, uint64_t* offsets,
                             uint64_t offsets_bytes, lt_hip_hit* items, uint64_t items_bytes);

/* Box-overlap queries: the primitives an axis-aligned box touches, their number, or whether there is any -- for voxelisers and
 * occupancy grids, the broad phase of a collision check against a volume, region selection, binning a scene into bricks.
 *
 * Record: lt_hip_box {lo[3], pad0, hi[3], pad1}; the pads are ignored.  A box is EMPTY, and touches nothing, when any of its six
 * bounds is not finite or lo[k] <= hi[k] fails on some axis; lo == hi is a valid point box.
 * Candidates: the leaves of the caller's LinearBVHNode array, each with its one primitive, exactly as the nearest queries take
 * them; a leaf with primitiveCount > 1 contributes that one primitive once.
 * A candidate touches the box q iff both hold:
 *   boxes_meet     q meets the leaf's own box as the caller gave it: per axis q.lo <= leaf.hi && leaf.lo <= q.hi.  A NaN bound
 *                  makes it false.
 *   tri_meets_box  the traversal triangle as the scene stores it, A, e1 = fl(B - A), e2 = fl(C - A), is separated from q by none
 *                  of 13 axes.  Every operation is one IEEE float32 operation rounded once, in the order given; nothing is
 *                  contracted, subnormals are kept.  A compare with a NaN is false, which reads "not separated".  min and max of
 *                  three are chains of compares: m = first; if (second < m) m = second; if (third < m) m = third (`>` for max).
 *     box axes (3)   un-centred, on the vertices A, fl(A + e1), fl(A + e2): axis k separates iff min > hi[k] or max < lo[k].
 *                    Compares only: a vertex exactly on a face touches the cells on both sides.
 *     centring       per axis c = 0.5 lo + 0.5 hi, h = 0.5 hi - 0.5 lo (two products, then the sum or difference; h >= 0),
 *                    v0 = A - c, v1 = v0 + e1, v2 = v0 + e2.
 *     plane (1)      n = e1 x e2: n.x = e1.y e2.z - e1.z e2.y, n.y = e1.z e2.x - e1.x e2.z, n.z = e1.x e2.y - e1.y e2.x;
 *                    d = (n.x v0.x + n.y v0.y) + n.z v0.z; r = (|n.x| h.x + |n.y| h.y) + |n.z| h.z; separates iff d > r or d < -r.
 *     edge axes (9)  the edges f0 = e1, f1 = e2 - e1, f2 = -e2 in that order, each crossed with the unit axes x, y, z in that
 *                    order.  The projections of v0, v1, v2 (in that order, all three) and the box's radius are
 *                      x:  p = v.z f.y - v.y f.z,   r = h.z |f.y| + h.y |f.z|
 *                      y:  p = v.x f.z - v.z f.x,   r = h.x |f.z| + h.z |f.x|
 *                      z:  p = v.y f.x - v.x f.y,   r = h.y |f.x| + h.x |f.y|
 *                    and the axis separates iff min(p) > r or max(p) < -r.  A point triangle or a needle gives zero axes, which
 *                    separate nothing; the other axes decide.
 *                  (lens_trace_amd/csrc/lt_overlap.hpp is the expression sequence; tests/overlap.py restates it in numpy.)
 * The sequence of a box: every touching candidate once, by ascending primitive offset, then ascending node index in the caller's
 * array (only scenes whose leaves name one primitive twice have a second key).  An empty box has the empty sequence.  The
 * sequence is a function of the scene and the box alone: whichever hierarchy is walked, the words are these.
 *   LT_OVERLAP_FIRST_K  the first max_k entries as max_k consecutive int32 primitive offsets per box, box-major: word
 *                       i * max_k + j is entry j of box i.  Unused slots hold -1.  No subtree can be skipped because of its
 *                       offsets, so this costs what LT_OVERLAP_COUNT costs.
 *   LT_OVERLAP_COUNT    one uint32 per box: the length of the sequence.
 *   LT_OVERLAP_ANY      one uint32 per box: 1 iff the sequence is not empty (the walk may stop at the first touch).
 *
 * flags: 0.  max_k: 1 .. LT_OVERLAP_MAX_K for LT_OVERLAP_FIRST_K, 0 for the other kinds.  Host memory, synchronous.  Errors in
 * lt_hip_nearest_k's order: LT_ERR_INVALID_ARGUMENT for a null ctx / desc, struct_size too small, flags != 0, an unknown kind,
 * max_k outside its range for the kind, n >= 2^32, a null pointer with n > 0 (and, device entry point, pointers that are not
 * 16-byte aligned); LT_ERR_NO_SCENE; LT_ERR_BUFFER_TOO_SMALL when out_bytes < 4 max_k n (FIRST_K) or 4 n (COUNT, ANY).  A failed
 * call writes nothing to out; n == 0 launches nothing.  lt_hip_get_stats then reports rays = n, kernel_launches = 1 and
 * kernel_ms.  (lens_trace_amd/csrc/lt_overlap.hip) */
#define LT_OVERLAP_FIRST_K 0
#define LT_OVERLAP_COUNT   1
#define LT_OVERLAP_ANY     2
#define LT_OVERLAP_MAX_K   8
typedef struct lt_hip_box { float lo[3]; uint32_t pad0; float hi[3]; uint32_t pad1; } lt_hip_box;   /* 32 B */
typedef struct lt_hip_overlap_desc {
  uint32_t struct_size;         /* >= sizeof(lt_hip_overlap_desc) */
  uint32_t flags;               /* 0 */
  int32_t kind;                 /* LT_OVERLAP_FIRST_K / LT_OVERLAP_COUNT / LT_OVERLAP_ANY */
  uint32_t max_k;               /* FIRST_K: 1 .. LT_OVERLAP_MAX_K; COUNT, ANY: 0 */
} lt_hip_overlap_desc;          /* 16 B */

int lt_hip_overlap_boxes(lt_hip_context* ctx, const lt_hip_overlap_desc* desc, const lt_hip_box* boxes, uint64_t n,
                         void* out, uint64_t out_bytes);
/* Device memory of the context's GPU, enqueued on hip_stream (a hipStream_t, NULL = default stream), not waited for. */
int lt_hip_overlap_boxes_device(lt_hip_context* ctx, const lt_hip_overlap_desc* desc, const lt_hip_box* boxes, uint64_t n,
                                void* out, uint64_t out_bytes, void* hip_stream);
/* The same answers on the host, without a context or a GPU, from the caller's buffers, as lt_hip_nearest_k_host takes them: a scan
 * of the caller's leaves in node order.  LT_ERR_INVALID_ARGUMENT (a null desc, struct_size, flags, kind or max_k as above, a null
 * or mis-sized buffer, n >= 2^32), LT_ERR_BAD_SCENE (a leaf whose offset lies outside prims), LT_ERR_BUFFER_TOO_SMALL; a failed
 * call writes nothing. */
int lt_hip_overlap_boxes_host(const void* nodes, uint64_t node_bytes, const void* prims, uint64_t prim_bytes,
                              const lt_hip_overlap_desc* desc, const lt_hip_box* boxes, uint64_t n, void* out, uint64_t out_bytes);

/* Triangle-overlap queries: the primitives a query triangle meets, their number, or whether there is any -- the narrow phase of
 * a collision check (a moving mesh, a swept polygon), cutting planes, portal quads; a needle is a segment query and a point
 * triangle a point-on-surface query.  With rays, spheres (the nearest queries) and boxes this completes the query shapes.
 *
 * Record: lt_hip_tri {a[3], pad0, b[3], pad1, c[3], pad2}: the vertices P, Q, R; the pads are ignored.  A query is EMPTY, and
 * meets nothing, when any of its nine coordinates is not finite.  A degenerate triangle is valid.
 * Candidates: the leaves of the caller's LinearBVHNode array, each with its one primitive, exactly as the box queries take them.
 * A candidate touches the query iff both hold:
 *   boxes_meet     the query's box meets the leaf's own box as the caller gave it (lt_hip_overlap_boxes' boxes_meet), with
 *                  qbox.lo[k] = min3(P[k], Q[k], R[k]), qbox.hi[k] = max3(P[k], Q[k], R[k]) by that call's compare chains.
 *   tri_meets_tri  none of 17 axes separates the traversal triangle as the scene stores it, A, e1 = fl(B - A), e2 = fl(C - A),
 *                  from the query.  Every operation is one IEEE float32 operation rounded once, in the order given; nothing is
 *                  contracted, subnormals are kept.  A compare with a NaN is false, which reads "not separated".  Everything is
 *                  seen from P:
 *     terms          g1 = Q - P, g2 = R - P, d = A - P; the scene's vertices s0 = d, s1 = d + e1, s2 = d + e2; the query's +0,
 *                    g1, g2.  Edges f0 = e1, f1 = e2 - e1, f2 = -e2 and h0 = g1, h1 = g2 - g1, h2 = -g2.
 *                    cross(a, b) = (a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x); dot = (x x' + y y') + z z'.
 *     axes (17)      in this order: n = cross(e1, e2); m = cross(g1, g2); the nine cross(f_i, h_j), i-major; cross(n, f_i),
 *                    i = 0..2; cross(m, h_j), j = 0..2.  The last six lie in the two planes and decide coplanar pairs.
 *     per axis a     ps = (dot(a, s0), dot(a, s1), dot(a, s2)), pq = (+0, dot(a, g1), dot(a, g2)); the axis separates iff
 *                    (min3(ps) > max3(pq) or max3(ps) < min3(pq)) and the five dot products are all finite.  A zero axis
 *                    separates nothing; an axis whose arithmetic overflowed to inf or NaN separates nothing (that is what the
 *                    finiteness clause is for: the compare chains keep their first operand against a NaN); one that underflowed
 *                    to zero separates nothing.
 *                  At the magnitude limits (coordinates near 2^40 or 2^-40) the in-plane axes, products of four lengths, degrade
 *                  first -- they overflow or underflow and drop out -- and the answer stays conservative: more touches, never
 *                  fewer than the axes that survive allow.
 *                  A query whose first vertex P equals a vertex of a primitive bit for bit touches that primitive whenever
 *                  boxes_meet holds: P = A gives s0 = 0; P = B gives s1 = fl(fl(A - B) + fl(B - A)) = 0 exactly, likewise P = C;
 *                  so both projection sets contain 0 on every axis.
 *                  (lens_trace_amd/csrc/lt_tritri.hpp is the expression sequence; tests/overlap_tris.py restates it in numpy.)
 * The sequence of a query: every touching candidate once, by ascending primitive offset, then ascending node index.  Kinds,
 * descriptor and output words are lt_hip_overlap_boxes': LT_OVERLAP_FIRST_K (max_k int32 offsets per query, -1 in unused slots),
 * LT_OVERLAP_COUNT, LT_OVERLAP_ANY (one uint32 per query).
 *
 * flags: 0.  Host memory, synchronous.  Errors and their order are lt_hip_overlap_boxes': LT_ERR_INVALID_ARGUMENT for a null ctx /
 * desc, struct_size too small, flags != 0, an unknown kind, max_k outside its range for the kind, n >= 2^32, a null pointer with
 * n > 0 (and, device entry point, pointers that are not 16-byte aligned); LT_ERR_NO_SCENE; LT_ERR_BUFFER_TOO_SMALL when
 * out_bytes < 4 max_k n (FIRST_K) or 4 n (COUNT, ANY).  A failed call writes nothing to out; n == 0 launches nothing.
 * lt_hip_get_stats then reports rays = n, kernel_launches = 1 and kernel_ms.  (lens_trace_amd/csrc/lt_tritri.hip) */
typedef struct lt_hip_tri { float a[3]; uint32_t pad0; float b[3]; uint32_t pad1; float c[3]; uint32_t pad2; } lt_hip_tri;   /* 48 B */

int lt_hip_overlap_tris(lt_hip_context* ctx, const lt_hip_overlap_desc* desc, const lt_hip_tri* tris, uint64_t n,
                        void* out, uint64_t out_bytes);
/* Device memory of the context's GPU, enqueued on hip_stream (a hipStream_t, NULL = default stream), not waited for. */
int lt_hip_overlap_tris_device(lt_hip_context* ctx, const lt_hip_overlap_desc* desc, const lt_hip_tri* tris, uint64_t n,
                               void* out, uint64_t out_bytes, void* hip_stream);
/* The same answers on the host, without a context or a GPU, from the caller's buffers, as lt_hip_overlap_boxes_host takes them: a
 * scan of the caller's leaves in node order.  Errors as lt_hip_overlap_boxes_host's; a failed call writes nothing. */
int lt_hip_overlap_tris_host(const void* nodes, uint64_t node_bytes, const void* prims, uint64_t prim_bytes,
                             const lt_hip_overlap_desc* desc, const lt_hip_tri* tris, uint64_t n, void* out, uint64_t out_bytes);

/* Overlap lists: the WHOLE sequence of every box or query triangle, as CSR -- what a voxeliser, a brick binner or a narrow phase
 * needs where LT_OVERLAP_FIRST_K stops at eight.  Queries, candidates, "touches" and the sequence are lt_hip_overlap_boxes' and
 * lt_hip_overlap_tris', word for word.
 *   offsets   n + 1 uint64: offsets[i] is the sum of the sequence lengths of queries 0 .. i-1 (an exclusive scan: offsets[0] = 0,
 *             offsets[n] the total).
 *   items     offsets[n] int32: items[offsets[i] .. offsets[i + 1]) is the sequence of query i -- every touching candidate's
 *             primitive offset, ascending (then by node index: the words being offsets only, this is the sorted multiset).  An
 *             empty query has an empty segment.
 * So the differences of offsets are LT_OVERLAP_COUNT's words and the first eight of a segment LT_OVERLAP_FIRST_K's.
 * Sizing: items == NULL with items_bytes == 0 writes the offsets only and returns LT_OK.  With items and
 * items_bytes < 4 offsets[n], NOTHING is written to items, offsets is written in full and valid, and the host-memory forms return
 * LT_ERR_BUFFER_TOO_SMALL -- the one exception to "a failed call writes nothing".  The device form cannot know and returns LT_OK:
 * its caller reads offsets[n].
 * flags: 0, or LT_OVERLAP_LIST_FLAG_FILL_ONLY: offsets is INPUT -- what an earlier call returned for the same scene and records
 * -- and only items is written, so that a sized-then-filled pair of calls costs two walks of the hierarchy and not three.
 * Whatever those offsets hold, nothing is written outside items[0 .. items_bytes / 4): query i writes only into
 * [offsets[i], min(offsets[i + 1], items_bytes / 4)), and a length that would be negative is 0.  With offsets that are not this
 * batch's own the words are unspecified, but in bounds.
 * Cost: the count is LT_OVERLAP_COUNT's walk, the fill that walk again; each segment is then sorted by one wavefront, up to 4096
 * entries in LDS and longer ones in place in device memory -- a segment of a million entries is slow, but correct.
 * Errors, in lt_hip_overlap_boxes' order: LT_ERR_INVALID_ARGUMENT for a null ctx / desc, struct_size too small, an unknown flag,
 * n >= 2^32, null records or offsets with n > 0, items == NULL with items_bytes != 0, LT_OVERLAP_LIST_FLAG_FILL_ONLY with
 * items == NULL (and, device entry point, pointers that are not 16-byte aligned); LT_ERR_NO_SCENE; LT_ERR_BUFFER_TOO_SMALL when
 * offsets_bytes < 8 (n + 1).  Such a call writes nothing.  n == 0 writes offsets[0] = 0 (not with FILL_ONLY) and launches nothing.
 * lt_hip_get_stats then reports rays = n, kernel_ms and the kernels launched: 4 for the sizing call (walk, three of the scan),
 * 2 for FILL_ONLY (walk, ordering), 6 for both.  (lens_trace_amd/csrc/lt_overlist.hip) */
#define LT_OVERLAP_LIST_FLAG_FILL_ONLY 0x1u
typedef struct lt_hip_overlap_list_desc {
  uint32_t struct_size;         /* >= sizeof(lt_hip_overlap_list_desc) */
  uint32_t flags;               /* 0 / LT_OVERLAP_LIST_FLAG_FILL_ONLY */
} lt_hip_overlap_list_desc;     /* 8 B */

int lt_hip_overlap_boxes_list(lt_hip_context* ctx, const lt_hip_overlap_list_desc* desc, const lt_hip_box* boxes, uint64_t n,
                              uint64_t* offsets, uint64_t offsets_bytes, int32_t* items, uint64_t items_bytes);
/* Device memory of the context's GPU, enqueued on hip_stream (a hipStream_t, NULL = default stream), not waited for. */
int lt_hip_overlap_boxes_list_device(lt_hip_context* ctx, const lt_hip_overlap_list_desc* desc, const lt_hip_box* boxes, uint64_t n,
                                     uint64_t* offsets, uint64_t offsets_bytes, int32_t* items, uint64_t items_bytes, void* hip_stream);
/* The same lists on the host, without a context or a GPU, from the caller's buffers, as lt_hip_overlap_boxes_host takes them: a
 * scan of the caller's leaves in node order, sorted per query.  Errors as above, with lt_hip_overlap_boxes_host's for the scene
 * (LT_ERR_BAD_SCENE where the context's entry points have LT_ERR_NO_SCENE). */
int lt_hip_overlap_boxes_list_host(const void* nodes, uint64_t node_bytes, const void* prims, uint64_t prim_bytes,
                                   const lt_hip_overlap_list_desc* desc, const lt_hip_box* boxes, uint64_t n, uint64_t* offsets,
                                   uint64_t offsets_bytes, int32_t* items, uint64_t items_bytes);
int lt_hip_overlap_tris_list(lt_hip_context* ctx, const lt_hip_overlap_list_desc* desc, const lt_hip_tri* tris, uint64_t n,
                             uint64_t* offsets, uint64_t offsets_bytes, int32_t* items, uint64_t items_bytes);
int lt_hip_overlap_tris_list_device(lt_hip_context* ctx, const lt_hip_overlap_list_desc* desc, const lt_hip_tri* tris, uint64_t n,
                                    uint64_t* offsets, uint64_t offsets_bytes, int32_t* items, uint64_t items_bytes, void* hip_stream);
int lt_hip_overlap_tris_list_host(const void* nodes, uint64_t node_bytes, const void* prims, uint64_t prim_bytes,
                                  const lt_hip_overlap_list_desc* desc, const lt_hip_tri* tris, uint64_t n, uint64_t* offsets,
                                  uint64_t offsets_bytes, int32_t* items, uint64_t items_bytes);

/* Statistics of the most recent render call or ray query on ctx (waits for it to finish). */
int lt_hip_get_stats(lt_hip_context* ctx, lt_hip_stats* out);

/* Camera-hit passes launched on ctx since it was created.  accumulator walks the camera rays of a call of two or more frames in a
 * pass ahead of its render launches and keeps the hits: a call with the same scene, camera, image, tile set and math flavour as the
 * one before it -- a progressive caller moving frame_first on -- launches no pass and this number stays.  LT_CAMERA_HITS_KEEP=0:
 * every such call launches one.  Waits for nothing; 0 for a null ctx. */
uint64_t lt_hip_camera_hit_passes(const lt_hip_context* ctx);

/* Entry cuts: with the camera hits accumulator keeps, per 8x8 square, a list of nodes of its own tree (fifteen to a record) that
 * the square's shadow rays towards the lights can reach at all, and the two-frame shadow walks of the square start there instead
 * of at the root -- same pixels.  The first call that reuses a set of kept hits builds the lists, later ones reuse them; a call
 * that runs its own camera-hit pass builds none (but for the one call that times the shadow walks).  out3[0]: builds on ctx so
 * far; out3[1], out3[2]: squares with a non-empty list and the entries of those lists, of the cuts ctx holds now.  Waits for the
 * context's last render.  LT_ENTRY_CUT=0: no cuts are built and every walk starts at the root. */
int lt_hip_entry_cut_counts(lt_hip_context* ctx, uint64_t* out3);

/* The entry cut's interval test on the host, for tests: n cases of (origin: 3 floats, the light primitives' vertex box before it is
 * pushed outwards: lo xyz hi xyz, a node's box: lo xyz hi xyz).  out[i]: 0 no half-line from the origin towards a point of the
 * light box meets the node's box, 1 one may, 2 the lane is one the cut is not built for (non-finite or huge values).  No GPU. */
int lt_hip_entry_cut_test_host(const float* origins, const float* light_boxes, const float* boxes, uint64_t n, uint8_t* out);

/* The leaf pass of the entry cuts: after the node lists, the build tests the triangles of the leaves a square's rays can
 * reach against the shaft of lines from its stored camera hits towards the light box.  Where it finishes within its budget of
 * records and at most a list's worth of leaves survive, those leaves replace the square's list -- or, where none survives, the
 * square is marked clear and its two-frame shadow walks are not run at all.  Same pixels.  out3[0]: squares marked clear, out3[1]:
 * squares whose list is leaves, out3[2]: the entries of those lists, of the cuts ctx holds now (lt_hip_entry_cut_counts keeps
 * describing the node lists the pass started from).  Waits for the context's last render.  LT_ENTRY_CUT_LEAVES=0: node lists only,
 * (0, 0, 0); LT_ENTRY_CUT_LEAVES=N, N >= 2: the budget of records per square, for measurements (default 512). */
int lt_hip_entry_cut_leaf_counts(lt_hip_context* ctx, uint64_t* out3);

/* Lists of several records: a square's list may take up to N 64-byte records of at most fifteen entries, which the
 * square's two-frame shadow walk goes through one after the other with the rays that are still unoccluded -- a list of leaves up to
 * LT_ENTRY_CUT_CHUNKS=N records, 1 .. 16 (default 16; 1: one record per list, as before there were several), a list of nodes up to
 * LT_ENTRY_CUT_NODE_CHUNKS=M of them, M <= N (default 2).  Same pixels.  The two calls above keep their meaning: lt_hip_entry_cut_counts counts the node
 * lists, however long, and lt_hip_entry_cut_leaf_counts the lists of leaves that fit one record.  Where the leaf pass finishes with more
 * surviving leaves than a list holds, the list is a cut over the tree as the pass saw it, without the subtrees in which no leaf
 * survived, instead of a node list chosen by box reach alone.  A value of M above N counts as N.  The lists take 64 bytes times N per
 * 8x8 square of device memory in the context (1 KiB per square at the default N: 133 MB at 4K).
 * Of the cuts ctx holds now: out23[0] the N they were built with; out23[1], out23[2] the squares whose list is leaves in more than one
 * record, and the entries of those lists; out23[3], out23[4] the squares whose list is a cut over the pruned tree, and its entries;
 * out23[5], out23[6] the squares whose list stays a node list of more than one record, and its entries; out23[6 + k], k = 1 .. 16, the
 * squares whose list, of any kind, takes k records.  Waits for the context's last render. */
int lt_hip_entry_cut_chunk_counts(lt_hip_context* ctx, uint64_t* out23);

/* Diagnostics: copies the entry cuts ctx holds now back to the host, as the two-frame shadow walks read them (tests say from them
 * what their walks ran through): one plane per record a square's list may take (out23[0] above), each plane 16 uint32 per 8x8 square
 * of the image the cuts were built for, in hand-out order -- a count, 0 .. 15, or 0xffffffff for a square marked clear, then that many
 * references in the walk's stack encoding (bit 31 set: a leaf's record among lt_hip_read_scene_structure's kind 4).  A record after the
 * first with a count of 0 ends its square's list.  out == NULL: only *out_bytes (the size) is set.  *out_bytes = 0 while the context
 * holds no cuts: no call has reused a set of camera hits yet, or they were dropped since (another scene, camera or image).  Waits for
 * the device. */
int lt_hip_read_entry_cuts(lt_hip_context* ctx, void* out, uint64_t capacity, uint64_t* out_bytes);

/* The cut over the pruned tree on the host, for tests: a tree of n <= 512 records as the leaf pass writes it down (record 0 the root;
 * refs[v] negative: a leaf; parents[v], kids[2 v], kids[2 v + 1]: record indices, 0xffff none) and survives[v] != 0 for the leaves that
 * survive.  out: the references of the cut, at most cap (2 .. 240) of them; *count: their number.  No GPU. */
int lt_hip_entry_cut_pruned_test_host(const uint32_t* refs, const uint16_t* parents, const uint16_t* kids, const uint8_t* survives, uint32_t n,
                                      uint32_t cap, uint32_t* out, uint32_t* count);

/* The arithmetic of those records on the host, for tests: n cases of (the own tree's height, the N asked for, a list's entries, a
 * record's index).  out[4 i ..]: the entries one record holds under that height (0: no lists), the entries a list may have, the
 * records this list takes, and the count of the record with that index.  No GPU. */
int lt_hip_entry_cut_chunks_test_host(const int32_t* heights, const uint32_t* chunks, const uint32_t* entries, const uint32_t* which, uint64_t n,
                                      uint32_t* out);

/* The leaf pass's triangle test on the host, for tests: n cases of (origin: 3 floats, the light primitives' vertex box before it is
 * pushed outwards: lo xyz hi xyz, a traversal triangle as the walks' leaf records hold it: v0, v1 - v0, v2 - v0).  out[i]: 0 no
 * line through the origin towards a point of the light box passes the float triangle test in any math flavour, 1 one may, 2 the
 * lane is one the cut is not built for.  No GPU. */
int lt_hip_entry_cut_triangle_test_host(const float* origins, const float* light_boxes, const float* triangles, uint64_t n, uint8_t* out);

/* random()'s short sine on the host, for tests (lt_device.hpp: random_fast_r, the same operation sequence as the kernels').  n
 * cases, either of (uvx, uvy, seed) in args3 -- the argument formed as math flavour `flavour` (0 portable, 1 device libm, 2 as
 * shipped) forms it and reduced by fmod_pi -- or, where r is not null, of that reduced argument itself.  params10, where not
 * null, replaces the eight coefficients, pi_lo and delta (tests of mutated copies).  Out, each nullable: r_out the reduced
 * argument, p the fast value of sin(r) * 43758.5453, determined 1 where the float is proved to be the library's, a that float
 * (before the fract).  No GPU. */
int lt_hip_random_fast_test_host(int flavour, const float* args3, const double* r, uint64_t n, const double* params10, double* r_out,
                                 double* p, uint8_t* determined, float* a);

/* Clear squares handed out whole.  A call that reuses a camera's entry cuts hands its squares out from an item
 * table built behind the cuts, on the device: a square marked clear is one work item for all frames of the launch instead of one
 * per frame group, and where the launch is a fused one of a depth-3 image whose tile width is a multiple of 8, without padded
 * tiles and with a 16-byte aligned output, that item folds its samples into the running mean itself, frame by frame: they are neither
 * stored nor read back by the fold.  Same pixels.  LT_CLEAR_ITEMS=0: the hand-out and the fold as they were without it.
 * The table is taken only where it thins the hand-out: the build's counters come back to the host asynchronously, and once they are
 * there a set of cuts with fewer than a third of its squares clear is rendered without the table, as before there was one (the
 * Cornell box at 4K lost 0.15 ms to it).  LT_CLEAR_ITEMS=1: the table however few squares are clear; =2: likewise, and whole squares
 * store their samples (the hand-out alone, for measurements).
 * Of the table ctx holds now: out5[0] its entries and out5[1] the squares it hands out whole, as the build counted them; out5[2] those
 * of them that the host told some launch of the context's last render call to fold that way (all or none: the host's decision, not a
 * count by the render kernel); out5[3] the tables built so far; out5[4] 1 if some launch of the last render call took the table.
 * Waits for the context's last render. */
int lt_hip_clear_item_counts(lt_hip_context* ctx, uint64_t* out5);

/* A clear square handed out whole renders its two-frame groups in one pass over the square: the per-pixel set-up once, two new
 * randoms per group (a group shares two seeds with the next), the running mean in registers where the square folds.  A group whose
 * frames would not walk together, or with a light sample off the light list, and a trailing group of one frame go back to the
 * per-group path.  Same pixels.  LT_CLEAR_SQUARE=0: every group through the per-group path.
 * Of the context's last render launch, as its waves counted: out3[0] the squares that entered the pass, out3[1] those of them that left
 * it before their last group, out3[2] the frame groups rendered in it.  All zero where the launch took no such pass.  Waits for the
 * context's last render. */
int lt_hip_clear_square_counts(lt_hip_context* ctx, uint64_t* out3);

/* The item table and its fold map on the host, for tests: marks[p] is word 0 of the list of the square at hand-out position p < n
 * (0xffffffff: clear), order[p] that square's index (NULL: p), groups the frame groups of the launch.  table: 16 + n * groups
 * words -- words 0 .. 7 the entry counts of the eight shares, the entries of share x from word 16 + (start of x) * groups, an entry
 * (place in the share) * groups + group, bit 31 set for a whole square.  map (NULL: none): one byte per 8-pixel row segment of
 * tiles_in_call stacked tiles of tile_w x tile_h pixels (tile_w a multiple of 8; n their 8x8 squares), 1 in a whole square.  No GPU. */
int lt_hip_clear_items_test_host(const uint32_t* marks, const uint32_t* order, uint32_t n, uint32_t groups, uint32_t tile_w, uint32_t tile_h,
                                 uint32_t tiles_in_call, uint32_t* table, uint8_t* map);

#ifdef __cplusplus
}
#endif
#endif /* LENSTRACE_HIP_H */
