// bl_kernel_plan.h - which kernel instantiation each stage of a render runs. Host only: no kernel reads it and it is part of no argument
// block. PlanKernels (bl_render.hip) fills it from the render's plan, once; every bl_launch_* wrapper takes its part, maps it to a
// function pointer through one selector per kernel family, checks that the argument block agrees, and launches that pointer. The
// fields are the kernels' template arguments, in the kernels' order.
#ifndef BLACKLIGHT_AMD_BL_KERNEL_PLAN_H_
#define BLACKLIGHT_AMD_BL_KERNEL_PLAN_H_

struct KernelPlan {
  // bl_ray_init_kernel<true, spin_zero> (the fixed-step steppers start from the Dormand-Prince instantiation and leave the first-stage
  // derivatives it also writes unread) and bl_geodesic_kernel<integrator, with_time, spin_zero, shell> (spin_zero: Dormand-Prince only;
  // shell: ... without sample times only). source: who fills the chunk's records - only kStepper launches the geodesic kernel.
  struct Geodesic {
    enum Source { kStepper, kCheckpoint, kResident } source = kStepper;
    int integrator = 0;
    bool with_time = false, spin_zero = false, shell = false;
    // The proper distance of the stepper's stages (no template argument: BlTraceArgs::distance_mode, wave-uniform at run time). kNone: no
    // stepper runs, or a fixed-step one, which has no distance; kExact: the reference's operations; kClosed: bl_distance_closed.h
    enum Distance { kNone, kExact, kClosed } distance = kNone;
  } geodesic;
  // bl_geodesic_quad_kernel<spin_zero> behind the stepper (BL_TAIL_QUAD) or beside it, after bl_split_long_kernel (BL_TAIL_SPLIT)
  struct Quad {
    bool park = false, split = false, spin_zero = false;
  } quad;
  // bl_locate_plain_kernel<spin_zero>, or bl_locate_kernel<refined, slow, false, tables_in_hbm>
  struct Locate {
    enum Kind { kNone, kPlain, kGeneral } kind = kNone;
    bool spin_zero = false, refined = false, slow = false, tables_in_hbm = false;
  } locate;
  // the coefficient kernel. kShade: bl_shade_kernel<model, aux, extended, sks, polarized, false>; kExact: bl_shade_exact_kernel<spin_zero>;
  // kFast: bl_shade_fast_kernel<spin_zero, mode>; kFormulaFast: bl_shade_formula_fast_kernel; kFused2: bl_shade_fused2_kernel<spin_zero,
  // composed, factors, refined>; kExact2: bl_shade_exact2_kernel<spin_zero>; kPolarized2: bl_shade_polarized2_kernel<spin_zero, records,
  // coefficients>
  struct Shade {
    enum Family { kShade, kExact, kFast, kFormulaFast, kFused2, kExact2, kPolarized2 } family = kShade;
    int model = 0, mode = 0;
    bool spin_zero = false, aux = false, extended = false, sks = false, polarized = false;
    bool composed = false, factors = false, refined = false, records = false, coefficients = false;
  } shade;
  // the exact second pass behind kFast, kFormulaFast and kFused2: bl_shade_kernel<model, false, extended, sks, false, spin_zero, true>
  // with table_bytes of dynamic LDS (the mesh's tables behind the fused kernel over a mesh with inter-block interpolation)
  struct Redo {
    bool run = false;
    int model = 0, table_bytes = 0;
    bool extended = false, sks = false, spin_zero = false;
  } redo;
  // per-frequency kernels: bl_polarized_coefficients_kernel<false, thermal_only> (not with the coefficients inside kPolarized2),
  // bl_polarized_frame_kernel (every polarized run), bl_coefficients_freq_kernel<true>
  struct PerFrequency {
    bool polarized_coefficients = false, thermal_only = false, polarized_frames = false, coefficients_freq = false;
  } freq;
  // the transfer kernel: bl_transfer_aux_kernel, bl_transfer_freq_kernel, bl_transfer_composed_kernel, bl_transfer_quad_kernel or
  // bl_transfer_kernel<affine> (a lane per ray and frequency); tau: bl_tau_kernel behind it
  struct Transfer {
    enum Kind { kAux, kFreq, kComposed, kQuad, kLane } kind = kLane;
    bool affine = false, tau = false;
  } transfer;
  // polarized transfer: bl_transfer_polarized_kernel (tensor transport along the ray), or bl_transport_matrix_kernel and
  // bl_transfer_polarized_matrix_kernel - in sequence, or the matrices on the second stream beside the per-frequency coefficients
  enum PolarizedRoute { kUnpolarized, kTensor, kMatrix, kMatricesBeside } polarized = kUnpolarized;
};

// Where a stage that finds a sample's cell reads the grid's coordinate tables, and the launch that follows from their size. One helper
// beside each launch wrapper fills it (bl_locate_tables, bl_shade_inside_tables, bl_shade_redo_tables); the wrapper launches from what the
// helper returned and the `tables:` debug line prints the same values (DescribeTables, bl_render.hip).
struct TableLaunch {
  // kNone: the stage does not run or finds no cells; kLds: tables staged in LDS; kHbm: searched where they lie in HBM; kLocated: the
  // stage reads the samples a locate kernel left
  enum Where { kNone, kLds, kHbm, kLocated } where = kNone;
  int table_bytes = 0;     // kLds: bytes of tables staged
  size_t lds_bytes = 0;    // dynamic LDS of the launch: the tables and what lies behind them
  int raise_to = 0;        // > 0: hipFuncAttributeMaxDynamicSharedMemorySize asked for before the launch
  int lanes = 256, blocks = 0;
  int grid = 0;            // the count of 256-lane workgroups the render asked for, from which `blocks` follows
};

#endif  // BLACKLIGHT_AMD_BL_KERNEL_PLAN_H_
