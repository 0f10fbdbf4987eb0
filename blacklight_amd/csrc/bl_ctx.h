// bl_ctx.h - the context behind the C-ABI handle (include/blacklight_amd.h) and the few helpers the host-side
// translation units of the HIP path share: bl_api.hip (construction, validation, grid upload, settings),
// bl_render.hip (bl_render: chunk planning, kernel pipeline, statistics), bl_grid.cpp (a grid's tables) and bl_checkpoint.cpp (the
// checkpoint files and their conversions) - the last two host code only. Internal, hidden visibility.
#ifndef BLACKLIGHT_AMD_BL_CTX_H_
#define BLACKLIGHT_AMD_BL_CTX_H_
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <limits>
#include <map>
#include <memory>
#include <mutex>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/blacklight_amd.h"
#include "bl_bessel.h"
#include "bl_camera.h"
#include "bl_device.h"
#include "bl_grid.h"
#include "bl_internal.h"
#include "bl_refine.h"

// The launch wrappers (at the end of each kernel file): each takes its part of the render's KernelPlan (bl_kernel_plan.h), maps it to a
// kernel through one selector per kernel family, and returns hipErrorInvalidValue where the argument block disagrees with the choice
extern "C" hipError_t bl_launch_ray_init(const BlTraceArgs *args, const KernelPlan::Geodesic &plan, hipStream_t stream);
extern "C" hipError_t bl_launch_geodesic(const BlTraceArgs *args, const KernelPlan::Geodesic &plan, int grid, hipStream_t stream, int lds_pad);
extern "C" int bl_geodesic_occupancy(const KernelPlan::Geodesic &plan);
extern "C" hipError_t bl_launch_geodesic_quad(const BlTraceArgs *args, const KernelPlan::Quad &plan, int grid, hipStream_t stream, int lds_pad);
extern "C" hipError_t bl_launch_split_long(const BlTraceArgs *args, hipStream_t stream);
extern "C" hipError_t bl_launch_locate(const BlShadeArgs *args, const KernelPlan::Locate &plan, int grid, int lds_bytes, hipStream_t stream);
extern "C" hipError_t bl_launch_shade(const BlShadeArgs *args, const KernelPlan::Shade &plan, int grid, hipStream_t stream);   // kShade, kExact
extern "C" hipError_t bl_launch_shade_fast(const BlShadeArgs *args, const KernelPlan::Shade &plan, int grid, hipStream_t stream);
extern "C" hipError_t bl_launch_shade_formula_fast(const BlShadeArgs *args, int grid, hipStream_t stream);
extern "C" hipError_t bl_launch_shade_fused2(const BlShadeArgs *args, const KernelPlan::Shade &plan, int grid, hipStream_t stream);
extern "C" hipError_t bl_launch_shade_exact2(const BlShadeArgs *args, const KernelPlan::Shade &plan, int grid, hipStream_t stream);
extern "C" hipError_t bl_launch_shade_polarized2(const BlShadeArgs *args, const KernelPlan::Shade &plan, int grid, hipStream_t stream);
extern "C" hipError_t bl_launch_shade_redo(const BlShadeArgs *args, const KernelPlan::Redo &plan, int grid, hipStream_t stream);
// (where each stage that finds cells reads the coordinate tables, and its launch: what the wrappers above launch from, TableLaunch)
extern "C" void bl_locate_tables(const BlShadeArgs *args, const KernelPlan::Locate &plan, int grid, int lds_bytes, TableLaunch *out);
extern "C" void bl_shade_inside_tables(const BlShadeArgs *args, const KernelPlan::Shade &plan, int grid, TableLaunch *out);   // kFused2, kExact2, kPolarized2
extern "C" void bl_shade_redo_tables(const BlShadeArgs *args, const KernelPlan::Redo &plan, int grid, TableLaunch *out);
extern "C" int bl_fused2_applicable(const BlGridDevice *grid, int n_nu, long long n_rays);
extern "C" int bl_fused2_refined_applicable(const BlGridDevice *grid, int n_nu, long long n_rays);
extern "C" int bl_polarized2_refined_applicable(const BlGridDevice *grid, long long n_rays);
extern "C" hipError_t bl_launch_polarized_coefficients(const BlShadeArgs *args, const KernelPlan::PerFrequency &plan, int grid, hipStream_t stream);
extern "C" hipError_t bl_launch_polarized_frames(const BlShadeArgs *args, int grid, hipStream_t stream);
extern "C" hipError_t bl_launch_coefficients_freq(const BlShadeArgs *args, int grid, hipStream_t stream);
extern "C" hipError_t bl_launch_transfer(const BlTransferArgs *args, const KernelPlan::Transfer &plan, hipStream_t stream);
extern "C" hipError_t bl_launch_tau(const BlTransferArgs *args, hipStream_t stream);
extern "C" hipError_t bl_launch_transfer_polarized(const BlTransferArgs *args, hipStream_t stream);
extern "C" hipError_t bl_launch_transport_matrices(const BlTransferArgs *args, int num_cus, hipStream_t stream);
extern "C" hipError_t bl_launch_transfer_polarized_rays(const BlTransferArgs *args, hipStream_t stream);
extern "C" hipError_t bl_launch_refine(const BlRefineArgs *args, hipStream_t stream);   // bl_refine_kernel (bl_refine.hip)
extern "C" hipError_t bl_launch_debug_math(int op, long long n, const double *x, const double *y, double *out, hipStream_t stream);

namespace blhost {

constexpr double kPi = 3.141592653589793;
constexpr double kC = 2.99792458e10;
constexpr double kGGMsun = 1.32712440018e26;
constexpr double kMp = 1.67262192369e-24;
constexpr double kMe = 9.1093837015e-28;   // (the kernels' values: bl_kernel_util.h)
constexpr double kE = 4.80320425e-10;
constexpr double kSqrt2 = 1.4142135623730951;
constexpr int kNumCellValues = 7;

struct Failure {
  int code;
  std::string message;
};

// Owning HBM allocation. Freed by the destructor (bl_free selects the context's device before it deletes the
// context, so every buffer a context holds - scratch sets, grid, time slices, block tables - goes back to the
// device); movable (the slow-light window swaps slices), not copyable.
template <typename T>
struct DeviceBuffer {
  T *ptr = nullptr;
  size_t count = 0;
  DeviceBuffer() = default;
  DeviceBuffer(const DeviceBuffer &) = delete;
  DeviceBuffer &operator=(const DeviceBuffer &) = delete;
  DeviceBuffer(DeviceBuffer &&other) noexcept : ptr(other.ptr), count(other.count) {
    other.ptr = nullptr;
    other.count = 0;
  }
  DeviceBuffer &operator=(DeviceBuffer &&other) noexcept {
    if (this != &other) {
      Free();
      ptr = other.ptr;
      count = other.count;
      other.ptr = nullptr;
      other.count = 0;
    }
    return *this;
  }
  ~DeviceBuffer() { Free(); }
  uint64_t Bytes() const { return count * sizeof(T); }
  void Free() {
    if (ptr != nullptr) (void)hipFree(ptr);
    ptr = nullptr;
    count = 0;
  }
  void Ensure(size_t n) {
    if (n <= count) return;
    Free();
    hipError_t err = hipMalloc(reinterpret_cast<void **>(&ptr), n * sizeof(T));
    if (err != hipSuccess)
      throw Failure{BL_E_DEVICE, std::string("hipMalloc of ") + std::to_string(n * sizeof(T)) + " bytes failed: " + hipGetErrorString(err)};
    count = n;
  }
};

inline void Check(hipError_t err, const char *what) {
  if (err != hipSuccess) throw Failure{BL_E_DEVICE, std::string(what) + ": " + hipGetErrorString(err)};
}

}  // namespace blhost
using namespace blhost;

// One image of a render: an electron model (R_low, R_high), a density unit (simulation_rho_cgs), a sigma cut (cut_sigma_max) and an
// electron mix. ResolveVariants gives every variant all four - the parameter block's where a setter stored none (what the setters
// store of an axis that is not theirs is zero and not read).
struct Variant {
  double rat_low, rat_high, rho, sigma_max;
  bl_electron_mix mix;
};
// Where a variant lies on the four axes: electron mix e, model m, unit u, sigma cut s
struct VariantPlace {
  int e, m, u, s;
};
// The mixes of bl_ctx::mixes that one render covers: [begin, end), clipped to the list - by default all of it - and whether that
// render runs a shading pass per variant whatever its variants could share (bl_render: a list rendered as several runs).
struct MixRange {
  int begin = 0, end = std::numeric_limits<int>::max();
  bool pass_per_variant = false;
};
// A render's variants, in image-row order and never empty (ResolveVariants): the product electron mixes x models x units x sigma
// cuts of an unpolarized run, or the triples of a polarized one.
// n_mixes ... n_cuts and n_pol are the axes as set, 0: the parameter block's - what refusals and file tags ask. `extent` is the shape
// as rendered, every axis at least 1. Index and At are the one place that knows the row order, v = ((e M + m) U + u) S + s; its
// device-side counterpart, which must agree, is the channel decode of bl_transfer_freq_kernel (bl_transfer.hip).
// Polarized triples are one flat axis of their own, with a pair, a unit, a cut and a mix per triple. It stands where the cuts stand:
// extent = (1, 1, 1, n_pol) and triple t lies at (0, 0, 0, t), which is what the plan wants of it - a BlShadeCold block per cut is
// then a block per triple (PlanVariantCuts).
struct Variants {
  std::vector<Variant> list;
  int n_models, n_units, n_pol, n_cuts, n_mixes;
  VariantPlace extent;
  int Index(int e, int m, int u, int s) const { return ((e * extent.m + m) * extent.u + u) * extent.s + s; }
  VariantPlace At(int v) const {
    const int pair = v / extent.s, model = pair / extent.u;
    return {model / extent.m, model % extent.m, pair % extent.u, v % extent.s};
  }
};

struct bl_ctx {
  bl_params params;
  bl_camera_frame frame;
  BlSpacetime st;
  std::vector<double> frequencies;   // what every render, query and writer reads: bl_set_frequencies' list, else the parameter block's
  int frequencies_set = 0;           // ... the list's length, 0: the block's own (BuildFrequencies); its size() is the frequency count everywhere
  std::string last_error, warnings;
  int device = 0;
  int num_cus = 256;
  hipStream_t stream = nullptr;       // shading stream: locate, coefficient and transfer kernels, uploads
  hipStream_t stream_geo = nullptr;   // geodesic kernel of the next chunk, concurrent with the above
  // BL_SWITCH_SPLIT_LONG: two streams whose CU masks partition the device - split_cus compute units for bl_geodesic_quad_kernel
  // and the rays predicted long, the rest for bl_geodesic_kernel (hipExtStreamCreateWithCUMask)
  hipStream_t stream_few = nullptr, stream_most = nullptr;   // (borrowed from a process-wide table, never destroyed: bl_render.hip)
  int split_cus_made = 0;             // compute units of the quad stepper's stream as it exists (an eighth of the device)
  int split_lds_pad = 39 * 1024;      // LDS a wave of either stepper reserves so that a CU takes four of them, one per SIMD
  bool split_unavailable = false;     // the runtime refused a CU-masked stream: BL_TAIL_AUTO stops asking
  std::vector<hipEvent_t> events;     // kEventsPerChunk per scratch set + begin / end of the render
  unsigned long long *host_counters = nullptr;   // pinned, BL_CNT_TOTAL per scratch set
  uint64_t scratch_limit = 144ull << 30;
  int overlap_chunks = 0;             // bl_set_overlap(): geodesic kernel of chunk c + 1 beside the shading of chunk c
  int arithmetic = BL_ARITH_TOLERANT; // bl_set_arithmetic(); BLACKLIGHT_AMD_ARITHMETIC = exact | tolerant sets what a new context starts with
  int reproducible = 0;               // bl_set_reproducible(): tolerant tier without composed transfer maps
  int tail_policy = BL_TAIL_AUTO;     // bl_set_tail_policy()
  hipStream_t caller_stream = nullptr;   // bl_set_caller_stream(): work queued there before a bl_render call precedes its kernels
  bool caller_stream_set = false;
  hipEvent_t caller_event = nullptr;
  int undefined_policy = BL_UNDEFINED_REFUSE;   // bl_set_undefined_policy(): BL_UNDEFINED_EDGE | BL_UNDEFINED_KAPPA
  bool kappa_warned = false;
  bool debug_counters = false;        // BLACKLIGHT_AMD_DEBUG_COUNTERS (bl_init): print the -DBL_GEO_STATS counters after a render
  unsigned int switches = 0;          // BL_SWITCH_* (include/blacklight_amd.h): the environment as bl_init found it, never read again
  double guard_band = 1.0e-9;         // tolerant tier: relative half-width around a cut threshold left to the exact kernel

  // image rows (radiation_integrator.cpp:436-520)
  int image_num_quantities = 0;      // of one electron model and unit (bl_image_num_quantities: times the number of each)
  // what the four setters stored, empty: the parameter block's - bl_set_electron_models() pairs (rho unused), bl_set_density_units()
  // units (the pair unused), bl_set_polarized_variants() triples, bl_set_sigma_cuts() thresholds; read through ResolveVariants only
  std::vector<Variant> models, units, triples;
  bool triples_cut = false;          // the triples carry a cut_sigma_max each (bl_set_polarized_variants_sigma); else the parameter block's
  bool triples_mix = false;          // ... and an electron mix each (bl_set_polarized_variants_electrons); else the parameter block's
  std::vector<double> sigma_cuts;
  std::vector<bl_electron_mix> mixes;   // bl_set_electron_mixes(): the outermost axis of an unpolarized run's variants; empty: the parameter block's mix
                                        // (written by StoreElectronMixes alone: a render reads the part of it that its MixRange names)
  // bl_set_cameras(): the viewing angles as given (degrees) and each camera's frame; empty: the parameter block's camera. `frame`
  // above is what a one-camera render starts its rays from - the block's own frame (block_frame), or the one camera of a list of
  // one, so that such a render plans and runs exactly as a context with those angles in its block; two cameras or more reach the
  // kernels through d_cameras (BlTraceArgs::cameras), uploaded when the list changes.
  struct Camera {
    double th_deg, ph_deg;
    bl_camera_frame frame;
  };
  std::vector<Camera> cameras;
  bl_camera_frame block_frame;
  DeviceBuffer<BlCameraDevice> d_cameras;
  bool cameras_uploaded = false;
  int tile_order_cameras = 0;        // cameras d_tile_order interleaves (with tile_order_res, tile_order_xcd)
  BlAuxImages aux_images{};          // which image rows exist; .any = an auxiliary image or a rendering is requested
  int render_num_images = 0;         // false-colour renderings (0 in formula mode)
  DeviceBuffer<BlRenderDevice> d_render_params;
  DeviceBuffer<double> d_render;     // staging for host output
  double plasma_thermal_frac = 0.0;

  // bl_set_grid beside bl_render (another host thread: the next snapshot of a series staged while this one renders). The render holds
  // render_lock from start to end; a bl_set_grid whose geometry is the one in place uploads its cells into d_cells_back on a stream of
  // its own without the lock, then takes it - waiting for the render to end - to let the two cell arrays change places.
  std::mutex render_lock;
  // The grid as bl_set_grid left it: what the host built of the caller's description (bl_grid.h), the device's copy of each table, and
  // the kernels' view of both. A refused or failed bl_set_grid leaves `have` false.
  struct Grid {
    bool have = false;
    bool swappable = false;            // d_cells was filled as tables.placement says, and d_cells_back may take its place (not so for a time slice of slow light)
    bl_grid_desc meta{};               // the description's scalars (its pointers were the caller's, for the duration of the call)
    GridTables tables;                 // host tables, placement, extents, budgets, the geometry as given and its hash (0: none kept)
    BlGridDevice dev{};                // tables.dev with every pointer bound to the buffers below
    DeviceBuffer<float> d_cells, d_cells_back;
    DeviceBuffer<float> d_cell_planes;                 // the caller's eight variable planes as uploaded, before bl_interleave_cells_kernel
    DeviceBuffer<unsigned long long> d_block_origin;   // ... and where every block's cells go in a merged array
    DeviceBuffer<float> d_kappa;       // electron entropy per cell (plasma_model = code_kappa)
    DeviceBuffer<double> d_coords;
    DeviceBuffer<unsigned short> d_buckets;
    DeviceBuffer<int> d_lattice;       // refined mesh: box of the block-boundary lattice -> block, the blocks' rows
    DeviceBuffer<unsigned int> d_fused_desc;   // ... -> what bl_shade_fused2_kernel<..., kRefined> needs of the block (BlGridDevice::fused_desc)
    DeviceBuffer<double> d_sks_map;    // simulation_coord = fmks: the reader's SKS -> FMKS look-up table
    DeviceBuffer<int> d_block_table;                  // inter-block interpolation: levels, locations, hash blocks
    DeviceBuffer<unsigned long long> d_block_keys;    // ... and hash keys
    hipStream_t stream_upload = nullptr;
    hipEvent_t source_event = nullptr; // bl_set_grid_device with wait: recorded on the caller's stream, awaited by the staging stream
    int64_t host_bytes = 0;            // what the last bl_set_grid* call copied from host memory (bl_grid_host_bytes)
    DeviceBuffer<double> d_harm_points;            // bl_set_grid_device_harm: the point table of the grid whose serial is ...
    unsigned long long harm_points_serial = 0;     // ... this one (0: none)
  } grid;
  bool sample_checkpoint_saved = false;   // checkpoint_sample_save: written with the first image only (radiation_integrator.cpp:699-704)

  // slow light: the reader's window of time slices (prim[n], time[n]; n = 0 latest) on one geometry
  struct SlowSlice {
    DeviceBuffer<float> cells, kappa;
    double time = 0.0;
    bool set = false;
  };
  std::vector<SlowSlice> slow_slices;
  bl_slow_state slow_state{};            // reader-side bookkeeping of bl_slow_light_read (bl_snapshot.cpp)
  bool polarized = false;                // image_light and image_polarization in simulation mode
  int snapshot = 0;                      // index of the image being rendered (warning texts, camera time)
  long long stats_slow_count[4] = {0, 0, 0, 0};    // pixels needing extrapolation in the last render, by kind
  double stats_slow_val[4] = {0.0, 0.0, 0.0, 0.0};
  DeviceBuffer<unsigned long long> d_slow_table;   // cells pointers, kappa pointers, times, extrapolation maxima
  DeviceBuffer<unsigned int> d_ray_extrap;

  // Per-chunk scratch, two sets (the geodesic kernel fills one while the shading kernels drain the other when bl_set_overlap is
  // on). Every array has one entry per sample record or per kept sample, so a set holds `record_capacity` of each and a chunk
  // is as many rays as the geodesic kernel fits into it (BlTraceArgs::record_gate).
  struct ChunkSlot {
    DeviceBuffer<BlSampleHot> d_records_hot;
    DeviceBuffer<BlSampleCold> d_records_cold;
    DeviceBuffer<BlLocated> d_located;
    DeviceBuffer<unsigned long long> d_located_tag;
    DeviceBuffer<double2> d_transfer;
    DeviceBuffer<double2> d_composed;              // tolerant tier: one affine map per ray segment (BlShadeArgs::composed)
    DeviceBuffer<double> d_parked;                 // rays bl_geodesic_kernel leaves to bl_geodesic_quad_kernel (BlTraceArgs::parked)
    DeviceBuffer<unsigned long long> d_counters;   // BL_CNT_TOTAL
    DeviceBuffer<BlAuxSample> d_aux;               // auxiliary-image mode
    DeviceBuffer<double> d_sample_t;               // image_time, slow light
    DeviceBuffer<double> d_slow_frac;              // slow light: t_frac of every located sample
    DeviceBuffer<BlPolSample> d_pol_samples;       // polarized transfer
    DeviceBuffer<double> d_pol_matrix;             // tolerant tier: 12 doubles per sample
    DeviceBuffer<BlFreqInputs> d_freq_inputs;      // tolerant tier, several frequencies
    DeviceBuffer<double2> d_pol_coeffs;
    DeviceBuffer<double2> d_pol_variant_coeffs;    // polarized variants in one pass: [sample row][variant][n_nu][4] instead of d_pol_coeffs
    DeviceBuffer<unsigned int> d_anchors;          // inter-block interpolation: eight anchor cells per record
    DeviceBuffer<BlCoefInputs> d_coef_inputs;      // polarized runs: coefficient kernel -> polarized coefficient kernel
    DeviceBuffer<unsigned char> d_have_flags;      // ... where bl_shade_polarized2_kernel evaluates the coefficients itself: which records have them
    DeviceBuffer<unsigned long long> d_redo;       // tolerant tier: records left to the exact coefficient kernel
    DeviceBuffer<double> d_tau_inc;                // tolerant tier with an optical-depth image: alpha x length per sample and frequency
    DeviceBuffer<unsigned long long> d_xcd_state;  // trace order per XCD: queue heads, list lengths, cursors (BlTraceArgs::xcd_state)
    DeviceBuffer<unsigned int> d_xcd_lists;        // ... the record lists, BL_XCD_QUEUES of them
    // Every buffer of the set, once: what Bytes() and Free() fold over (a new buffer is declared above and named here)
    template <typename Slot, typename F>
    static void ForEach(Slot &s, F &&f) {
      f(s.d_records_hot); f(s.d_records_cold); f(s.d_located); f(s.d_located_tag); f(s.d_transfer); f(s.d_composed); f(s.d_parked); f(s.d_counters);
      f(s.d_aux); f(s.d_sample_t); f(s.d_slow_frac); f(s.d_pol_samples); f(s.d_pol_matrix); f(s.d_freq_inputs); f(s.d_pol_coeffs); f(s.d_pol_variant_coeffs);
      f(s.d_anchors); f(s.d_coef_inputs); f(s.d_have_flags); f(s.d_redo); f(s.d_tau_inc); f(s.d_xcd_state); f(s.d_xcd_lists);
    }
    uint64_t Bytes() const {
      uint64_t bytes = 0;
      ForEach(*this, [&bytes](const auto &buffer) { bytes += buffer.Bytes(); });
      return bytes - d_counters.Bytes();   // (the counters never were in this sum, which enters the scratch budget - PlanScratch - and so the capacities)
    }
    void Free() { ForEach(*this, [](auto &buffer) { buffer.Free(); }); }
  };
  ChunkSlot slot[2];
  // per ray of a bl_render call (indexed by traversal position; a chunk's kernels get pointers to its first ray): the arrays set aside with the resident records
  struct RayArrays {
    DeviceBuffer<double2> constants;   // (k_t, momentum factor): BlTraceArgs::ray_constants
    DeviceBuffer<int> sample_num, skipped, rows;
    DeviceBuffer<unsigned char> flags;
    DeviceBuffer<long long> out_index, offset;
    uint64_t Bytes() const { return constants.Bytes() + sample_num.Bytes() + skipped.Bytes() + rows.Bytes() + flags.Bytes() + out_index.Bytes() + offset.Bytes(); }
  };
  // bl_set_geodesic_reuse: the root level's geodesics as its last render left them (in one chunk, or in the kept layout below). The
  // buffers are the ones scratch set 0 and the
  // per-ray arrays below point at (`parked` false) or, while a render of another level works there, set aside in `store`
  // (`parked` true: that render allocates its own, which are set aside in turn when the root level comes back - two sets of
  // buffers that change places, no copy).
  struct ResidentGeodesics {
    bool valid = false, parked = false;
    bool super_tiles = false;                 // the tile order the records were traced in (bl_render.hip: BuildTraceArgs)
    bool mirror = false;                      // ... of the left half only: mirror pairs, every later frame shades them for both halves
    bool located_valid = false;               // ... and d_located / d_located_tag / d_anchors hold the samples as located on `geometry`
    std::vector<unsigned char> key;           // everything the records depend on (bl_render.hip: GeodesicKey)
    std::vector<unsigned char> located_key;   // ... and the located samples besides (LocatedKey)
    size_t record_capacity = 0;
    int tail_policy = BL_TAIL_WIDE;
    unsigned long long n_parked = 0, n_flagged = 0;
    unsigned long long counters[BL_CNT_TOTAL] = {};   // scratch set 0's counters as the geodesic (and locate) stage left them
    // Kept layout (a root level of more than one chunk): scratch set 0 is re-partitioned, nothing allocated. Its shading arrays serve one
    // chunk at a time with `record_capacity` entries; the store that holds every chunk's records is a list of segments - the record
    // arrays themselves and the tails of the shading arrays beyond `record_capacity` entries. One entry per chunk of the render that
    // integrated them: its first ray, its segment and where its records start there, its counters as its kernels left them. Empty: one
    // chunk, `counters` above.
    struct Segment {
      BlSampleHot *hot = nullptr;
      BlSampleCold *cold = nullptr;   // (null: interleaved, the cold half follows each hot one)
      double *sample_t = nullptr;
      size_t capacity = 0;            // records
    };
    struct Chunk {
      long long begin = 0;
      int segment = 0;
      size_t record_base = 0;
      unsigned long long counters[BL_CNT_TOTAL] = {};
    };
    std::vector<Segment> segments;
    std::vector<Chunk> chunks;
    int kept_n_nu = 0;   // the frequency count the kept layout was partitioned for: the shading arrays' share grows with it, into the store
    // A root-level render of more than one chunk whose records were not kept: its key and the records it used (including the
    // partly filled blocks). The next render with this key integrates in the kept layout, with a store sized from that count.
    bool pending = false;
    std::vector<unsigned char> pending_key;
    unsigned long long pending_records = 0;
    struct Buffers {
      DeviceBuffer<BlSampleHot> records_hot;
      DeviceBuffer<BlSampleCold> records_cold;
      DeviceBuffer<double> sample_t;
      DeviceBuffer<BlLocated> located;
      DeviceBuffer<unsigned long long> located_tag;
      DeviceBuffer<unsigned int> anchors;
      RayArrays rays;
      ChunkSlot slot;   // kept layout: the whole of scratch set 0 is set aside (its shading arrays hold part of the store)
      void Free() { *this = Buffers{}; }   // (every buffer's move assignment gives its memory back)
    } store;
  } resident;
  int geodesic_reuse = 1;             // bl_set_geodesic_reuse()
  RayArrays rays;
  DeviceBuffer<double> d_ray_start;              // BL_RAY_START_FIELDS rows: start state of every ray (bl_ray_init_kernel -> geodesic kernel); never set aside
  uint64_t RayBytes() const { return rays.Bytes() + d_ray_start.Bytes(); }
  DeviceBuffer<double> d_freq;
  DeviceBuffer<int> d_pixel_map, d_block_locs, d_tile_order;
  DeviceBuffer<int> d_refine_locs;               // bl_adaptive_refine_device: the level's block list ...
  DeviceBuffer<unsigned char> d_refine_flags;    // ... and its flags, grown as needed
  int tile_order_res = 0;
  bool tile_order_xcd = false;   // d_tile_order in super-tiles of 8 x 8 tiles (the trace order per XCD, bl_render.hip) or tile by tile
  // Mirror pairs (bl_render.hip: MirrorPairsApply). d_tile_order lists the left half's tiles only (tile_order_half), d_mirror_out holds, per
  // traced slot of that order, the output index of its mirror pixel. The camera check's verdict is kept with everything it depends on -
  // spacetime, camera frame, camera parameters, resolution (mirror_key): any change of those has it made again.
  bool tile_order_half = false;
  DeviceBuffer<long long> d_mirror_out;
  std::vector<unsigned char> mirror_key;
  bool mirror_ok = false;
  // Closed-form proper distance (bl_distance_closed.h): the geodesic keys (BuildReuseKeys) of the cameras whose frame had a step the
  // closed form did not decide and was rendered again. Fresh renders of such a camera go straight to the reference's operations.
  std::vector<std::vector<unsigned char>> distance_exact_keys;
  DeviceBuffer<BlShadeCold> d_shade_cold;
  DeviceBuffer<BlPolVariant> d_pol_variant_table;   // polarized variants in one pass: every variant's folded constants (BuildShadeArgs)
  std::vector<unsigned char> pol_variant_host;   // the bytes d_pol_variant_table holds
  DeviceBuffer<BlPolVariantArgs> d_pol_variant_args;   // ... and every variant's electron constants, where a mix has non-thermal electrons (BuildShadeArgs)
  std::vector<unsigned char> pol_variant_args_host;   // the bytes d_pol_variant_args holds
  std::vector<unsigned char> shade_cold_host;   // the bytes d_shade_cold holds (BuildShadeArgs uploads on change only)
  // host-output staging
  DeviceBuffer<double> d_image, d_camera_pos, d_camera_dir;
  DeviceBuffer<int> d_out_sample_num;
  DeviceBuffer<unsigned char> d_out_flags;

  // geodesic checkpoint of the root level (geodesic_checkpoint.cpp:28-108): what LoadGeodesics() read, by pixel
  struct Checkpoint {
    int num_steps = 0;
    double frame[7][4] = {};              // cam_x, u_con, u_cov, norm_con, norm_con_c, hor_con_c, vert_con_c as the file has them
    std::vector<double> frequencies;
    std::vector<double> camera_pos, camera_dir, factors;   // [n_pix][4], [n_pix][4], [n_pix]
    std::vector<uint8_t> flags;
    std::vector<int32_t> sample_num;
    std::vector<double> pos, dir, len;   // [n_pix][num_steps][4] x 2, [n_pix][num_steps]: reference order (far -> near)
  };
  // One loaded file serves every context of the process that names it (the command-line driver's one context per GPU: 67 GB at
  // 1024^2 once, not once per device): LoadGeodesicCheckpoint() keeps a process-wide table of weak references.
  std::shared_ptr<const Checkpoint> checkpoint;

  bl_stats stats{};
};

namespace blhost {
inline void Warn(bl_ctx *ctx, const std::string &message) { ctx->warnings += "Warning: " + message + "\n"; }
int Fail(bl_ctx *ctx, const Failure &failure);   // sets bl_last_error (or the global error when ctx is null), returns the code
void EnsureStreams(bl_ctx *ctx);
void DropResident(bl_ctx *ctx);   // the root level's kept geodesics go (bl_render.hip)
// (bl_api.hip) what bl_render's plan, bl_num_variants and bl_image_num_quantities read; `mixes`: the part of the mix list to resolve
Variants ResolveVariants(const bl_ctx *ctx, MixRange mixes = {});
inline bool UnitCut(const bl_params &p) {   // a cut the density unit enters is set: rho, n_e, p_gas or B
  return p.cut_rho_min >= 0.0 || p.cut_rho_max >= 0.0 || p.cut_n_e_min >= 0.0 || p.cut_n_e_max >= 0.0 || p.cut_p_gas_min >= 0.0 || p.cut_p_gas_max >= 0.0
      || p.cut_b_min >= 0.0 || p.cut_b_max >= 0.0;
}
// The parameter block's own electron mix, and a mix's thermal fraction (radiation_integrator.cpp:311: bl_init's expression)
inline bl_electron_mix BlockMix(const bl_params &p) {
  return bl_electron_mix{p.plasma_power_frac, p.plasma_p, p.plasma_gamma_min, p.plasma_gamma_max, p.plasma_kappa_frac, p.plasma_kappa, p.plasma_w, 0.0};
}
inline double ThermalFraction(const bl_electron_mix &mix) { return 1.0 - (mix.power_frac + mix.kappa_frac); }
inline bool ThetaECut(const bl_params &p) { return p.cut_theta_e_min >= 0.0 || p.cut_theta_e_max >= 0.0; }
const char *ElectronModelsRefusal(const bl_ctx *ctx, int n);   // bl_set_electron_models (bl_api.hip)
const char *DensityUnitsRefusal(const bl_ctx *ctx, int n);     // bl_set_density_units (bl_api.hip)
const char *PolarizedVariantsRefusal(const bl_ctx *ctx, int n);   // bl_set_polarized_variants (bl_api.hip)
const char *SigmaCutsRefusal(const bl_ctx *ctx, int n);        // bl_set_sigma_cuts (bl_api.hip)
const char *CamerasRefusal(const bl_ctx *ctx, int n);          // bl_set_cameras (bl_api.hip)
const char *ElectronMixesRefusal(const bl_ctx *ctx, int n, const bl_electron_mix *mix);   // bl_set_electron_mixes (bl_api.hip)
const char *FrequenciesRefusal(const bl_ctx *ctx, int n);      // bl_set_frequencies (bl_api.hip)
}  // namespace blhost

#endif  // BLACKLIGHT_AMD_BL_CTX_H_
