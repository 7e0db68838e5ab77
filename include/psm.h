/* psm.h -- C-ABI of the MI355X-native pressure-surrogate path ("libpsm_hip.so").
 *
 * Drop-in boundary for the surrogate call of the DLPoissonFoam solvers and the
 * Improved_SM evaluators of pauloacs/Solving-Poisson-s-Equation-through-DL-for-
 * CFD-apllications.  Paths below are relative to that repository.
 *
 *   PM  = Thesis_Work/Chapter5/parallelized/test_case/python_module.py
 *   PCI = Thesis_Work/Chapter5/parallelized/DLPoissonSolver/PythonComm_init.H
 *   PC  = Thesis_Work/Chapter5/parallelized/DLPoissonSolver/PythonComm.H
 *   SMD = Improved_SM/deltaU_to_deltaP/source/pressureSM_deltas/SM_call.py
 *   UGP = Improved_SM/U_to_gradP/evaluation/Eval_dual_Dense_onlycil.py
 *
 * Plain C types only: pointers, sizes, int status.  Every function returns
 * PSM_OK (0) or a negative error; the message is available from
 * psm_last_error().  Nothing here aborts the host solver (the reference
 * dereferences NULL on failure: PCI:11-18, log.DL:34-42).
 *
 * Ownership: the caller owns every buffer it passes; the library copies what
 * it needs before returning and never keeps a caller pointer (the reference
 * borrows the solver's buffer through PyArray_SimpleNewFromData, PC:17).
 * Threading: one in-flight call per handle; handles are independent.
 */
#ifndef PSM_H_
#define PSM_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PSM_ABI_VERSION 4

/* block layout + reassembly variant */
#define PSM_VARIANT_CHAPTER5 0 /* PM:303-332, 373-472 */
#define PSM_VARIANT_DELTAS   1 /* SMD:452-482, 182-365 */
#define PSM_VARIANT_GRADP    2 /* UGP:476-500, 255-369 */

/* scaling of the PCA coefficients around the network */
#define PSM_SCALER_MAX_ABS 0 /* PM:351,365; UGP:525,531; SMD:521-523,536-537 */
#define PSM_SCALER_STD     1 /* SMD:505-512,532-533 */
#define PSM_SCALER_MIN_MAX 2 /* SMD:513-520,534-535 */

/* arithmetic of the PCA contractions and the dense layers */
#define PSM_PRECISION_F32  0 /* exact-f32 MFMA (v_mfma_f32_32x32x2_f32) */
#define PSM_PRECISION_BF16 1 /* bf16 operands (bases, weights, activations), f32 accumulation (v_mfma_f32_32x32x16_bf16) */

#define PSM_OK               0
#define PSM_ERR_ARG         -1 /* invalid argument / shape */
#define PSM_ERR_STATE       -2 /* call order (model incomplete, no plan, ...) */
#define PSM_ERR_HIP         -3 /* a HIP runtime call failed */
#define PSM_ERR_NO_DEVICE   -4 /* no usable gfx950 device */
#define PSM_ERR_UNSUPPORTED -5 /* shape the reference itself cannot process */
#define PSM_ERR_NOMEM       -6
#define PSM_ERR_GEOMETRY    -7 /* a device-pointer solve ran on a grid whose flow-cell pattern is not the bound one */

/* intermediate results readable with psm_read_stage (parity tests) */
#define PSM_STAGE_X_INPUT    0 /* [rows, p_in]   scaled network input (PM:351)      */
#define PSM_STAGE_RES        1 /* [rows, p_out]  network output, inverse-scaled      */
#define PSM_STAGE_BLOCK_PRED 2 /* [rows, S*S*c_out] decoded blocks (PM:365-366)      */
#define PSM_STAGE_OFFSETS    3 /* [cases, c_out, B] per-block corrections (BC_coor)  */
#define PSM_STAGE_SHIFT      4 /* [cases, c_out] global shift (PM:472)               */
/* [rows, n_out(l)] output of hidden Dense layer l as the next launch read it (after a standalone LayerNormalization; before
 * one the next launch applies itself), rows in row-major order: stage PSM_STAGE_HIDDEN + l, 0 <= l < layers - 1.  Needs
 * keep mode (PSM_KEEP_HIDDEN=1 at psm_create: every hidden layer writes a buffer of its own; off by default). */
#define PSM_STAGE_HIDDEN    16

/* kernels of one solve, in launch order (psm_profile_solve) */
#define PSM_K_ENCODE   0
#define PSM_K_REDUCE   1
#define PSM_K_MLP      2 /* all dense layers together */
#define PSM_K_DECODE   3
#define PSM_K_STRIPS   4
#define PSM_K_CHAIN    5
#define PSM_K_PASTE    6
#define PSM_K_COUNT    7

typedef struct psm_handle psm_handle;

/* Replaces the module-level constants of PM:103-134,195,303-304 and the
 * Evaluation(...) constructor arguments of SMD:27 / UGP:31. */
typedef struct psm_config {
  int32_t abi_version;   /* PSM_ABI_VERSION */
  int32_t variant;       /* PSM_VARIANT_* */
  int32_t block;         /* S, block edge (128: PM:303, SMD "shape") */
  int32_t overlap;       /* overlap-strip width; 0 = variant default (12 / 32 / 96) */
  int32_t c_in;          /* input channels (3; 4 for pressureSM_Poisson) */
  int32_t c_out;         /* output channels (1; 2 for U_to_gradP) */
  int32_t p_in;          /* retained input PCs  (PM:113, SMD:87) */
  int32_t p_out;         /* retained output PCs (PM:112, SMD:86) */
  int32_t n_dense;       /* Dense layers including the linear head (PM:125-129) */
  int32_t scaler;        /* PSM_SCALER_* */
  int32_t sdf_channel;   /* channel whose non-zero cells are flow cells (2) */
  int32_t device;        /* HIP device ordinal */
  int32_t max_cases;     /* capacity of the case batch (>=1) */
  int32_t strict_degenerate; /* 1: keep NumPy semantics when the last block row
                                duplicates the previous one (NaN field, UGP:340);
                                0: leave that row out */
  int32_t precision;     /* PSM_PRECISION_* */
} psm_config;

/* ---- lifetime ------------------------------------------------------------ */
/* Replaces Py_Initialize + import python_module (PCI:3-18). */
int psm_create(const psm_config* cfg, psm_handle** out);
void psm_destroy(psm_handle* h);
/* Message of the last failure on `h` (or of the last failed psm_create when h is NULL). */
const char* psm_last_error(const psm_handle* h);

/* ---- model artefacts (PM:103-118,168-170; SMD:70-87,507-519) -------------- */
/* sklearn components_[:p] ([p, S*S*c] row-major) and mean_ ([S*S*c]). */
int psm_set_pca(psm_handle* h, const double* comp_in, const double* mean_in,
                const double* comp_out, const double* mean_out);
/* Keras Dense kernel [n_in, n_out] row-major and bias [n_out]; layer in [0, n_dense). */
int psm_set_dense(psm_handle* h, int32_t layer, int32_t n_in, int32_t n_out,
                  const float* kernel, const float* bias);
/* densePCA_attention ('MLP_attention' of utils.py:455-457; Improved_SM/deltaU_to_deltaP/source/pressureSM_deltas/NNs.py:40-72):
 *   x0 = relu(Dense(depth[0])(inputs));  a = LayerNormalization()(MultiHeadAttention(8, 64)(x0[:, None], x0[:, None]))[:, 0]
 *   for i in 1 .. n_layers-1:  x = relu(Dense(depth[i])(a));  a = LayerNormalization()(x + a)
 *   outputs = Dense(PC_p)(a)
 * maps onto n_dense = n_layers + 2 layers of this handle: layer 0 = the first Dense, layer 1 = the attention block
 * (psm_set_attention), layers 2 .. n_layers = the further Dense layers, the last layer = the head; psm_set_layernorm on layers
 * 1 .. n_layers (residual = 0 on layer 1, 1 behind the others).
 * psm_set_attention: the attention runs over a sequence of length 1 (NNs.py:54), so its softmax is exactly 1 and the query / key
 * projections do not enter the result: out = (x . Wv + bv) . Wo + bo.  Wv [d_model, n_heads, value_dim], bv [n_heads, value_dim]
 * (Keras `value` EinsumDense), Wo [n_heads, value_dim, d_model], bo [d_model] (`attention_output`), float32 row-major.  Folded
 * on the host (float64) into one affine layer without activation in Dense slot `layer` (0 < layer < n_dense - 1).
 * psm_set_layernorm: Keras LayerNormalization over the last axis behind hidden layer `layer` (call after that layer was set):
 *   act = (v - mean(v)) * rsqrt(var(v) + epsilon) * gamma + beta,   v = layer output (after its activation) [+ the layer's own
 *   input when residual != 0 -- NNs.py:64 `x + attn_output`; the layer must then be square], biased variance, float32;
 *   n = the layer's n_out, gamma / beta [n], epsilon > 0 (Keras default 1e-3).
 * Both: float32 and bf16 handles (the normalisation itself is float32 in both); the geometry-bound path is kept.  A
 * normalisation whose consumer is another hidden Dense layer costs no launch (that layer's launch applies it to its input rows);
 * the last one runs as its own small launch. */
int psm_set_attention(psm_handle* h, int32_t layer, int32_t d_model, int32_t n_heads, int32_t value_dim,
                      const float* Wv, const float* bv, const float* Wo, const float* bo);
int psm_set_layernorm(psm_handle* h, int32_t layer, int32_t n, const float* gamma, const float* beta, float epsilon,
                      int32_t residual);
/* conv1D_PCA head (NNs.py:75-124; architecture 'conv1D' of utils.py:452-454: 7 layers of 128-64-32-16-32-64-128 filters):
 * n_layers Conv1D layers (kernel_size taps, 'same' padding, ReLU) over the p_in scaled PCA coefficients seen as a sequence
 * [p_in, 1], then Flatten ([p_in, filters] row-major: index p * filters + c) and the Dense layers of psm_set_dense (the
 * reference has exactly one, Dense(PC_p)), the first of which takes p_in * filters inputs.  kernel [kernel_size, c_in,
 * c_out] float32 (Keras Conv1D layout; cross-correlation, (kernel_size - 1) / 2 zeros in front), bias [c_out]; layer in
 * [0, n_layers), c_in of layer 0 is 1.  Call for every layer BEFORE psm_set_dense(layer 0) and psm_plan_grid.  float32
 * handles only; such a model keeps the general (unbound) solve path unless it has a hidden Dense layer. */
int psm_set_conv1d(psm_handle* h, int32_t layer, int32_t n_layers, int32_t kernel_size, int32_t c_in, int32_t c_out,
                   const float* kernel, const float* bias);
/* max_abs: in_a[0] = max_abs_input_PCA, out_a[0] = max_abs_output_PCA (others ignored);
 * std: in_a = mean_in, in_b = std_in, out_a = mean_out, out_b = std_out  ([p_in]/[p_out]);
 * min_max: in_a = min_in, in_b = max_in, out_a = min_out, out_b = max_out. */
int psm_set_scaler(psm_handle* h, const double* in_a, const double* in_b,
                   const double* out_a, const double* out_b);

/* ---- geometry ------------------------------------------------------------ */
/* Fix the uniform grid shape (grid_shape_y/x of PM:216-217) and build the block
 * tables; the grid-native counterpart of init_func (PM:172-247). */
int psm_plan_grid(psm_handle* h, int32_t ny, int32_t nx);
/* Number of blocks per case of the current plan (len(x_list), PM:332). */
int psm_num_blocks(const psm_handle* h);
/* shape[4] = {ny, nx, c_in, c_out} of the current plan. */
int psm_grid_shape(const psm_handle* h, int32_t* shape);

/* Bind the geometry of the planned grid for the following solves -- the drop-in counterpart of the reference's
 * computeOnlyOnce / init_func split (SM_call.py:89-178, python_module.py:172-246: everything that depends on the
 * obstacle only is done once per simulation).  `grid` [ny, nx, c_in] float32 (host, or device memory when
 * on_device != 0): only its SDF channel (cfg.sdf_channel; flow cell = value != 0, SM_call.py:221) is read.
 * Every quantity the block-offset chain needs is a masked sum of decoded values, i.e. linear in the network
 * output with coefficients that depend on the masks and the model only; binding tabulates those coefficients, and
 * single-case solves then take 6 launches instead of 8: the strip means come from dot products with the last
 * hidden activation inside the head layer's launch, and the decode launch runs the offset chain and writes
 * value - offset - shift straight into the field (the decoded blocks are never stored; psm_read_stage(PSM_STAGE_PRED)
 * is stale while bound).  Same results as the unbound path up to float32 summation order.
 * CONTRACT: until psm_unbind_geometry / a new bind / a model or plan change, the SDF channel of every solved grid
 * must have the flow-cell pattern of the bound one; the other channels are free.  Case counts other than the bound
 * one keep the general path.
 * SDF FOLD (float32 handles, one bound case of at most 32 blocks, cfg.sdf_channel == c_in - 1; PSM_SDF_FOLD=0 in the
 * environment switches it off): the SDF channel's share of the PCA coefficients is computed once at the bind and the
 * encode of a bound solve contracts the other channels only.  The contract is then the SDF channel's VALUES: every
 * pixel of the solved grid's SDF channel must compare equal (float ==; a NaN on either side is a mismatch) to the
 * bound one.  The device check below compares the values in that case, with the same consequences.
 * The contract is CHECKED ON THE DEVICE at every bound solve: spare waves of the launch that computes the strip dots
 * compare the pattern of the grid being solved (one ballot per 64 pixels) with the bound one (with the SDF fold: also
 * its values with the bound SDF image).  On a mismatch the
 * solve's field is NaN everywhere -- never a plausible field of the wrong geometry -- and a flag in mapped pinned
 * memory is raised.  The host-buffer entries (psm_solve_grid, psm_wait_grid, psm_ring_wait) see the flag when the
 * solve has finished, drop the binding, solve the same grid again on the general path and return the correct
 * field with PSM_OK (psm_last_error tells, psm_guard_trips counts); after psm_solve_grid_device the NaN field is
 * what the caller gets and the next psm_synchronize returns PSM_ERR_GEOMETRY (binding dropped).  The riders use
 * CUs the head layer leaves idle; PSM_NO_GUARD=1 in the environment removes them (diagnostic).  bf16 handles: the decode rounds the network output to bf16, so their
 * strip dots are taken from the rounded output in a small launch of their own (7 launches; same rounding points as
 * the general bf16 path).  Grids of more than 64 blocks (the reference's shipped 400 x 3000 case has 104) take a
 * two-launch form of the end: one chain launch, then decode + paste in row chunks (7 launches instead of 9).
 * Returns PSM_ERR_UNSUPPORTED (nothing bound, solves unaffected) for configurations outside these paths: >= 64 block
 * columns, > 128 output components, no hidden layer, last hidden layer wider than 1024. */
int psm_bind_geometry(psm_handle* h, const float* grid, int32_t on_device);
/* The same for a case batch: grids [n_cases, ny, nx, c_in], one geometry per case slot.  Solves with exactly
 * n_cases cases (case i on geometry i) then take 7 launches instead of 9: head + strip dots, one chain launch
 * (a workgroup per case), decode + paste.  Other case counts keep the general path. */
int psm_bind_geometry_cases(psm_handle* h, const float* grids, int32_t n_cases, int32_t on_device);
int psm_unbind_geometry(psm_handle* h);
int psm_geometry_bound(const psm_handle* h);   /* 1 while a geometry is bound */
/* The flow-cell pattern that was bound: mask [bound cases][ny*nx] (1 = SDF channel != 0), for callers that want to check
 * the contract above on their side (cap = bytes available).  PSM_ERR_STATE when nothing is bound. */
int psm_bound_mask(const psm_handle* h, uint8_t* mask, size_t cap);
/* Number of solves so far whose grid was not the bound geometry (each dropped the binding). */
int64_t psm_guard_trips(const psm_handle* h);

/* ---- per-step solve: grid-native counterpart of py_func (PM:249-517) and of
 *      Evaluation.timeStep from block extraction to assemble_prediction
 *      (SMD:452-575, UGP:470-547) ------------------------------------------- */
/* Host buffers.  grid: [n_cases, ny, nx, c_in] float32 NHWC, already normalised
 * as at PM:288-297; fields: [n_cases, ny, nx, c_out].  out_scale: per-case factor
 * applied to the decoded blocks (max_abs_p*U_max^2, SMD:551) or NULL for 1.
 * Synchronous, like py_func. */
int psm_solve_grid(psm_handle* h, const float* grid, int32_t n_cases,
                   const float* out_scale, float* fields);
/* Host buffers, asynchronous: a ring of PSM_RING_SLOTS slots, each with its own pinned host buffers, device buffers,
 * scratch, stream and hipGraph (H2D copy -> kernels -> D2H copy = ONE graph replay per ticket), so the copies of
 * neighbouring tickets run on the DMA engines while another ticket's kernels compute (the reference's py_func is
 * synchronous, PM:249-517; this is the form for a caller that owns several independent cases or time steps, e.g. an
 * ensemble of PISO runs).  A slot must have been waited for before it comes round again: PSM_ERR_STATE if
 * PSM_RING_SLOTS tickets are already in flight.  A geometry bound with psm_bind_geometry applies to the ring as well.
 *
 * Three ways in, fastest first:
 *  (1) zero-copy: psm_ring_acquire hands out the next slot's pinned buffers; the caller packs its grid
 *      [n_cases, ny, nx, c_in] straight into *grid_in (the pack of PythonComm.H:2-9 written to pinned memory instead of
 *      `input_vals`), psm_ring_submit enqueues the ticket, psm_ring_wait returns when *fields_out
 *      [n_cases, ny, nx, c_out] holds the result.  *fields_out stays valid until the ticket that reuses the slot
 *      (PSM_RING_SLOTS tickets later) is submitted.
 *  (2) caller-registered memory: after psm_host_register(range) psm_submit_grid_io DMAs straight from `grid` and,
 *      when `fields` lies in a registered range too, straight into `fields` (psm_wait_grid(h, t, NULL) then only
 *      waits).  The caller keeps the ranges allocated until psm_host_unregister / psm_destroy and must not touch
 *      `grid` before the wait returns.  psm_solve_grid uses registered ranges the same way.
 *  (3) pageable memory: psm_submit_grid copies `grid` into the slot (the caller's buffer is free on return) and
 *      psm_wait_grid copies the field out. */
#define PSM_RING_SLOTS 8
int psm_ring_acquire(psm_handle* h, int64_t* ticket, float** grid_in, float** fields_out);
int psm_ring_submit(psm_handle* h, int64_t ticket, int32_t n_cases, const float* out_scale);
int psm_ring_wait(psm_handle* h, int64_t ticket);
/* Give an acquired ticket back without submitting it (the caller decided not to solve after all): its slot is free
 * again and is handed out when its turn comes round (slots rotate in ticket order).  PSM_ERR_ARG for a ticket that was
 * not acquired or was already submitted. */
int psm_ring_release(psm_handle* h, int64_t ticket);
int psm_host_register(psm_handle* h, void* ptr, size_t bytes);
int psm_host_unregister(psm_handle* h, void* ptr);
/* fields may be NULL (destination given to psm_wait_grid instead). */
int psm_submit_grid_io(psm_handle* h, const float* grid, int32_t n_cases, const float* out_scale, float* fields,
                       int64_t* ticket);
int psm_submit_grid(psm_handle* h, const float* grid, int32_t n_cases,
                    const float* out_scale, int64_t* ticket);
/* fields == NULL: the destination given to psm_submit_grid_io. */
int psm_wait_grid(psm_handle* h, int64_t ticket, float* fields);
/* Device buffers (HIP pointers on cfg.device), asynchronous on `stream`
 * (hipStream_t; NULL = the handle's own stream).  out_scale is a HOST pointer
 * (or NULL) read before return. */
int psm_solve_grid_device(psm_handle* h, const float* d_grid, int32_t n_cases,
                          const float* out_scale, float* d_fields, void* stream);
/* Reassembly alone (assemble_prediction, SMD:182 / UGP:255; correction loop PM:373-472)
 * of caller-supplied decoded blocks block_pred[B, S*S*c_out] for ONE case, host
 * buffers, synchronous.  grid supplies the flow mask (its sdf channel). */
int psm_reassemble(psm_handle* h, const float* grid, const float* block_pred, float* fields);
/* Evaluation only (a8): the label blocks of the planned layout with the per-block mean over the flow cells removed,
 *   y_array[b, ..., c][x_array[b, ..., sdf] != 0] -= mean(same selection)          (SMD:487-488, UGP:509-511)
 * grid [ny, nx, c_in] supplies the flow mask, labels [ny, nx, c_out] the label image(s); blocks_out
 * [B, S*S*c_out] has the layout psm_reassemble takes, so that labels -> psm_label_blocks -> psm_reassemble is the
 * reference's self-check of the assembly ("it should be almost perfect in that case", SMD:577-580; live form
 * UGP:546-547 test_dPdx / test_dPdy).  Host buffers, synchronous. */
int psm_label_blocks(psm_handle* h, const float* grid, const float* labels, float* blocks_out);
/* compute_in_block_error (Improved_SM/deltaU_to_deltaP/source/pressureSM_deltas/utils.py:210-243, called at SM_call.py:555-557):
 * the error of the DECODED BLOCKS of the last solve (case 0; on a bound geometry the blocks are decoded again from the stored
 * network output) against the label blocks, before any reassembly.  grid [ny, nx, c_in] = the grid that was solved (flow
 * cells: SDF channel != 0), labels [ny, nx, c_out] in the network's normalised output units; the label blocks are taken and
 * de-meaned like psm_label_blocks and multiplied by the solve's out_scale (SM_call.py:555: y_array * max_abs_p * U_max_norm^2).
 * Over the flow cells of all blocks, NaN differences left out, norm = max(true) - min(true):
 *   out[0] = mean(pred - true) / norm            (what the reference appends to pred_minus_true_block)
 *   out[1] = mean((pred - true)^2) / norm^2      (pred_minus_true_squared_block)
 *   out[2] = norm (norm_true), out[3] = max(pred) - min(pred) (norm_pred), out[4] = number of differences.
 * float64 accumulation; evaluation only (host buffers, synchronous). */
int psm_block_error(psm_handle* h, const float* grid, const float* labels, double* out);
/* ---- mesh-side entry: the contract of PythonComm_init.H / PythonComm.H ------------
 * psm_set_geometry installs the one-time tables that init_func builds (PM:195-243):
 *   vtx_m2g/wts_m2g [ny*nx,3]  simplices + barycentric weights, mesh -> grid (interp_weights, PM:210)
 *   indices         [ny*nx,2]  (ii, jj) image cell of every grid point (PM:233-241); points that
 *                              are outside the domain carry whatever the caller put there (the
 *                              reference: np.zeros in SMD:161, np.empty in PM:225) and are
 *                              scattered in order like the NumPy fancy assignment (last wins)
 *   sdfunct         [ny*nx]    signed-distance image (PM:227,240)
 *   vtx_g2m/wts_g2m [n_cells,3] grid -> mesh (PM:211); both NULL for a caller that only goes mesh -> grid
 *                              (the offline evaluators, SM_call.py:89-180): psm_solve is then refused
 *   maxs            [4]        max_abs_Ux, max_abs_Uy, max_abs_dist, max_abs_p (PM:109)
 *   normalise_sdf   0: SDF channel as is (PM:292), 1: divided by max_abs_dist (SMD:443)
 *   fill_input      0: interpolate (PM:280), 1: interpolate_fill (SMD:421-423)
 *   wall_threshold  cells whose interpolated SDF is below it keep the previous p (0.05, PM:494)
 * It also fixes the grid shape (psm_plan_grid).  psm_solve additionally requires c_in == 3, c_out == 1. */
int psm_set_geometry(psm_handle* h, int64_t n_cells, int32_t ny, int32_t nx,
                     const int32_t* vtx_m2g, const double* wts_m2g, const int32_t* indices,
                     const double* sdfunct, const int32_t* vtx_g2m, const double* wts_g2m,
                     const double* maxs, int32_t normalise_sdf, int32_t fill_input,
                     double wall_threshold);
/* init_func itself (PM:172-247; called through PythonComm_init.H:53-94 with the solver's cell array and the points of
 * its "top" and "obstacle" patches): builds the tables above IN C++ -- no interpreter, no SciPy -- and installs them
 * like psm_set_geometry.  cells [n,5] float64 = (Ux, Uy, Cx, Cy, p) (Ux decides which grid points are interpolable,
 * PM:231), top [n_top,2], obst [n_obst,2] boundary points; `rank` is accepted for signature compatibility (the MPI
 * gather of PM:179-185 stays with the caller).  psm_set_case supplies what the reference reads from files / hard-codes:
 * maxs[4] (the `maxs` file, PM:106-109), delta (5e-3, PM:195), every (boundary-point stride of the SDF, 10, PM:94-95),
 * wall_threshold (0.05, PM:494); defaults are those values with maxs = 1.
 * Differences from the SciPy-built tables (csrc/psm_geometry.cpp): (a) mesh -> grid: own Delaunay triangulation --
 * identical simplices and weights for points in general position; grid points OUTSIDE the hull of the cell centres
 * take the last simplex of the triangulator's list in both codes, which one that is differs (such points are
 * scattered into image cell (0,0) like the reference's zero-initialised `indices`, SMD:161 -- PM:225 leaves them
 * undefined); (b) grid -> mesh: the lattice is cut along fixed diagonals (every lattice square is cocircular: qhull's
 * choice is not reproducible).  A caller that needs qhull's very tables passes them to psm_set_geometry. */
int psm_set_case(psm_handle* h, const double* maxs, double delta, int32_t every, double wall_threshold);
int psm_init_geometry(psm_handle* h, const double* cells, int64_t n, const double* top, int64_t n_top,
                      const double* obst, int64_t n_obst, int32_t rank);
/* The table builder alone, host only (no GPU, no handle): psm_geometry_shape gives the grid shape (and optionally
 * bounds[4] = rounded x_min, x_max, y_min, y_max, PM:197-201) for sizing; psm_geometry_build fills caller-allocated
 * vtx_m2g/wts_m2g [ny*nx,3], indices [ny*nx,2], sdfunct [ny*nx], vtx_g2m/wts_g2m [n,3]. */
int psm_geometry_shape(const double* cells, int64_t n, double delta, int32_t* ny, int32_t* nx, double* bounds);
int psm_geometry_build(const double* cells, int64_t n, const double* top, int64_t n_top, const double* obst,
                       int64_t n_obst, double delta, int32_t every, int32_t* vtx_m2g, double* wts_m2g,
                       int32_t* indices, double* sdfunct, int32_t* vtx_g2m, double* wts_g2m);
const char* psm_geometry_last_error(void);
/* py_func (PM:249-517, serial form PM1:199-444): cells [n,5] float64 = (Ux, Uy, Cx, Cy, p) as
 * packed at PythonComm.H:2-9 -> p_out [n] float64 as read at PythonComm.H:31-36.  `rank` is
 * accepted for signature compatibility (the MPI funnel, PM:258/511, stays with the caller).
 * Synchronous. */
int psm_solve(psm_handle* h, const double* cells, int64_t n, int32_t rank, double* p_out);
/* The same in two halves, for ONE thread that advances several independent cases (one handle, i.e. one geometry and one
 * stream, per case -- the "ensemble of PISO cases" of a parameter study): psm_solve_begin copies `cells` (or DMAs from
 * the registered array) and enqueues the whole step, psm_solve_end waits for it and delivers p into the `p_out` given
 * to begin.  One step in flight per handle; psm_solve = begin + end. */
int psm_solve_begin(psm_handle* h, const double* cells, int64_t n, int32_t rank, double* p_out);
int psm_solve_end(psm_handle* h);
/* Optional: register the solver's own persistent buffers (the `input_vals` array of PythonComm_init.H:53 lives for the
 * whole run; the output array likewise) so that psm_solve DMAs from / to them directly instead of through the
 * handle's pinned staging copies (saves two host memcpys per step).  cells [n_cells,5] and / or p_out [n_cells] (either
 * may be NULL); the caller guarantees they stay allocated, at the same address, until psm_unpin_buffers, a new
 * psm_set_geometry or psm_destroy.  psm_solve calls with other pointers keep using the staging path.
 * With BOTH arrays registered (and up to 50 000 cells; above that the DMA engine's large-copy rate wins) a step issues no copy at all: the first kernel of the call reads `cells`
 * from the registered pages over PCIe (fully coalesced, taking the U_max partial maxima on the way) and the last one stores p
 * into `p_out` -- up to 9 us off the 74 us per call of the DMA-copy form on a 16 k-cell mesh, depending on the host's PCIe read
 * rates.  The caller must not
 * write `cells` or read `p_out` between psm_solve_begin and psm_solve_end. */
int psm_pin_buffers(psm_handle* h, const double* cells, double* p_out);
int psm_unpin_buffers(psm_handle* h);
/* ---- the solver boundary for a CASE BATCH: K meshes, one handle, one step ------------
 * The ensemble of PISO cases as one launch chain instead of one handle, stream and chain per case: K cases, each with its
 * own mesh and obstacle, all on ONE grid shape, advanced by one call -- per-case U_max (two-level device reduction, never on
 * the host), mesh -> grid for all cases, the batched solve, grid -> mesh for all cases.
 * psm_set_geometry_cases takes the tables of psm_set_geometry once per case: n_cells [n_cases] and n_cases pointers per
 * table (vertex indices address the case's own cells); maxs, normalise_sdf, fill_input and wall_threshold are shared.
 * All-or-nothing: every table is validated like psm_set_geometry's (the message names the case) before the handle is
 * touched; then the grid is planned, the per-case tables are uploaded and every per-step buffer is reserved (a step
 * allocates nothing).  Needs 1 <= n_cases <= max_cases (PSM_ERR_ARG), c_in == 3 and c_out == 1 (PSM_ERR_UNSUPPORTED) and
 * the grid -> mesh tables of every case (PSM_ERR_ARG).  Also accepted: the four-channel Poisson model (c_in == 4, c_out == 1,
 * sdf_channel == 3), with maxs = (max_abs_dUx, max_abs_dUy, max_abs_dist, max_abs_dp) as psm_set_geometry reads them for that
 * model; such a set binds no geometry and serves psm_bind_poisson_solve_cases / psm_solve_cases_poisson* alone:
 * psm_solve_cases*, psm_solve_cases_delta* and psm_delta_prime_cases on it are PSM_ERR_UNSUPPORTED.  And the gradP model
 * (c_in == 3, c_out == 2), with maxs = (max_abs_Ux, max_abs_Uy, max_abs_dist, unused): such a set binds its K geometries and serves
 * psm_bind_gradp_solve_cases / psm_solve_cases_gradp* alone, the three entries above are PSM_ERR_UNSUPPORTED on it too.
 * The K geometries are bound for this entry only (the scope
 * psm_set_geometry gives its one; a configuration outside the bound path solves on the general path; PSM_NO_BIND=1 keeps
 * the general path); with n_cases == 1 the route -- and every bit of p -- is that of psm_solve.
 * A handle holds EITHER the single mesh of psm_set_geometry OR a case set: setting one drops the other, psm_solve* on a case
 * set and psm_solve_cases* on a single mesh are PSM_ERR_STATE.  psm_plan_grid and the model setters drop the case set. */
int psm_set_geometry_cases(psm_handle* h, int32_t n_cases, const int64_t* n_cells, int32_t ny, int32_t nx,
                           const int32_t* const* vtx_m2g, const double* const* wts_m2g, const int32_t* const* indices,
                           const double* const* sdfunct, const int32_t* const* vtx_g2m, const double* const* wts_g2m,
                           const double* maxs, int32_t normalise_sdf, int32_t fill_input, double wall_threshold);
/* psm_init_geometry per case (tables built in C++ with the constants of psm_set_case), then psm_set_geometry_cases.
 * cells[k] [n[k],5], top[k] [n_top[k],2], obst[k] [n_obst[k],2].  PSM_ERR_ARG names the first case whose grid shape
 * differs from case 0's. */
int psm_init_geometry_cases(psm_handle* h, int32_t n_cases, const double* const* cells, const int64_t* n,
                            const double* const* top, const int64_t* n_top, const double* const* obst, const int64_t* n_obst);
/* One step of all cases.  The cell-side arrays are the cases' concatenated in case order: cells [sum n_i, 5] float64 ->
 * p [sum n_i] float64 (psm_mesh_cases gives the offsets).  A case's result does not depend on the other cases' cells.
 * _device: device pointers (8-byte aligned), asynchronous on `stream` (NULL: the handle's), copies nothing.
 * psm_solve_cases: host buffers, synchronous -- one H2D copy of the cells and one D2H copy of p, through the handle's
 * pinned staging or straight from / into ranges registered with psm_host_register.  _begin / _end: the same in two halves
 * (one step in flight per handle; a second begin, or an end without a begin, is PSM_ERR_STATE). */
int psm_solve_cases_device(psm_handle* h, const double* d_cells, double* d_p, void* stream);
int psm_solve_cases(psm_handle* h, const double* cells, double* p_out);
int psm_solve_cases_begin(psm_handle* h, const double* cells, double* p_out);
int psm_solve_cases_end(psm_handle* h);
/* The case set of the handle: *n_cases and cell_off [n_cases + 1] (either may be NULL).  PSM_ERR_STATE without one. */
int psm_mesh_cases(const psm_handle* h, int32_t* n_cases, int64_t* cell_off);
/* ---- the solver boundary in DELTA form: [U(t) - U(t-1)], SDF -> p(t) - p(t-1) ------------
 * The deltas model (pressureSM_deltas) behind the per-timestep call.  The reference evaluates it offline only and leaves the
 * dimensionalisation "when calling the SM in the CFD solver" (SM_call.py:548-551); these entries are that call.  A step takes
 * the cells [n,5] = (Ux, Uy, Cx, Cy, p) of psm_solve, where column 4 is p(t-1), and gives p(t):
 *   image     interpolate_fill((U(t) - U(t-1)) / U_max) / max_abs, the difference formed per cell in float64 (SM_call.py:389-391,
 *             418-419, 422-423, 432-443).  U_max = max sqrt(Ux^2 + Uy^2) of the CURRENT cells (:404, :417-419), not of the
 *             difference: the three ways psm_solve takes it.
 *   p_out[n]  cells[n][4] + field * max_abs_dp * U_max^2, and cells[n][4] BIT FOR BIT where psm_solve keeps the previous p
 *             (near-wall cell, negative weight, NaN: PM:494-496 applied to dp).
 * U(t-1) lives on the device ([sum n_i][2] float64, allocated with the geometry: a step allocates nothing).  The last launch of
 * a step stores the cells' (Ux, Uy) into it, so the state advances only when the whole step was enqueued, and a step makes
 * exactly the launches of psm_solve / psm_solve_cases on the same handle and route (bound, general, many-block).
 * Requirements, checks and error codes are those of psm_solve / psm_solve_cases (c_in == 3, c_out == 1, grid -> mesh tables,
 * matching cell count, single mesh or case set; the wrong kind is PSM_ERR_STATE).  The variant is not enforced: the layout is
 * the handle's.  `maxs` of the geometry call are read as (max_abs_dUx, max_abs_dUy, max_abs_dist, max_abs_dp); the deltas
 * model's convention is normalise_sdf = 1, fill_input = 1 (SM_call.py:441-443), which is the CALLER's to pass to
 * psm_set_geometry*: psm_init_geometry* keep passing 0, 0 -- a C++ host builds the tables with psm_geometry_build and hands them
 * to psm_set_geometry with 1, 1.
 * State: psm_delta_prime sets U(t-1) := cells[:,0:2] (no other column is read), psm_delta_reset forgets it and zeroes `steps`,
 * psm_delta_state reports *primed (0 / 1) and *steps, the delta steps taken since the state was last empty (either may be NULL).
 * A step on a state that is not primed is the PRIMING step: PSM_OK, p_out = cells[:,4] bit for bit, U(t-1) := cells[:,0:2],
 * `steps` not incremented, and the network does not run (its output for a zero image is not zero -- PCA means, biases -- so
 * "dU = 0" through the chain would move p): a solver's first call never aborts it.  Whatever drops the geometry or the case set
 * drops the state (a new psm_set_geometry*, psm_plan_grid, a model setter): psm_delta_state then reports primed = 0.
 * One step in flight per handle across both kinds: a delta begin while a psm_solve_begin is in flight, or the reverse, is
 * PSM_ERR_STATE, and either end completes the step that is in flight.  psm_solve* on the same handle neither reads nor moves
 * the state.  Registered buffers (psm_pin_buffers): the DMA-copy form, p stored straight into the registered output where
 * psm_solve does that; the one-kernel PCIe staging route of psm_solve is NOT taken by the delta entries.
 * NOT applied: the evaluator's "irrelevant time step" rule (SM_call.py:407-415) -- bookkeeping of its error metrics, no part of
 * the model -- and the Gaussian filter / dU weighting of assemble_prediction (psm_bind_poststeps has them). */
int psm_delta_prime(psm_handle* h, const double* cells, int64_t n);
int psm_delta_reset(psm_handle* h);
int psm_delta_state(const psm_handle* h, int32_t* primed, int64_t* steps);
int psm_solve_delta(psm_handle* h, const double* cells, int64_t n, int32_t rank, double* p_out);
int psm_solve_delta_begin(psm_handle* h, const double* cells, int64_t n, int32_t rank, double* p_out);
int psm_solve_delta_end(psm_handle* h);
/* The same for the case set of psm_set_geometry_cases, cell-side arrays concatenated in case order as for psm_solve_cases:
 * cells [sum n_i, 5] -> p [sum n_i]; one state for the set (all cases are primed and advance together).  _device: device
 * pointers (8-byte aligned), asynchronous on `stream` (NULL: the handle's), copies nothing; its priming step is one launch.
 * With n_cases == 1 every bit of p is psm_solve_delta's. */
int psm_delta_prime_cases(psm_handle* h, const double* cells);
int psm_solve_cases_delta_device(psm_handle* h, const double* d_cells, double* d_p, void* stream);
int psm_solve_cases_delta(psm_handle* h, const double* cells, double* p_out);
int psm_solve_cases_delta_begin(psm_handle* h, const double* cells, double* p_out);
int psm_solve_cases_delta_end(psm_handle* h);
/* Generic mesh -> grid step of the evaluators (interpolate_fill + scatter, SM_call.py:419-436,
 * pressureSM_Poisson/SM_call.py:580-600): values [n_cells, k] float64 row-major (k columns of cell
 * data) -> grid_out [ny*nx, k] float64 holding, per image cell, the interpolated value of the grid
 * point NumPy's `grid[...][tuple(indices.T)] = v` leaves there (last writer), 0 where nothing is
 * written; fill != 0: NaN where a barycentric weight is negative (utils.interpolate_fill).  Uses the
 * tables of psm_set_geometry.  Host buffers, synchronous. */
int psm_mesh_to_grid(psm_handle* h, const double* values, int64_t n_cells, int32_t k, int32_t fill, double* grid_out);

/* Input features of the pressureSM_Poisson surrogate (pressureSM_Poisson/SM_call.py:588-711): from the
 * interpolated dimensional grids ux, uy, dux, duy [ny,nx] float64 (zero outside the flow) and the raw
 * signed-distance image sdfunct [ny,nx] (0 inside solids) to the normalised grid image
 * grid_out [ny,nx,4] float32 = (arcsinh-smoothed Poisson source term, dUx/U, dUy/U, sdf), each divided by
 * its max_abs.  np.gradient differences masked at solid neighbours (:602-632), Poisson term (:635),
 * smart_arcsin_smooth_transform (:22-69, :646), NaN -> 0 (:704), rescale (:707-710).
 * params[7] = {L (= phi), U (= U_max_norm), k, max_abs_Poisson_term_1, max_abs_delta_Ux,
 * max_abs_delta_Uy, max_abs_dist}.  Host buffers, synchronous; the result feeds psm_solve_grid of a
 * deltas-variant handle with c_in = 4. */
int psm_poisson_features(psm_handle* h, const double* ux, const double* uy, const double* dux, const double* duy,
                         const double* sdfunct, int32_t ny, int32_t nx, const double* params, float* grid_out);
/* scipy.ndimage.gaussian_filter(field, sigma=(sigma_y, sigma_x), order=0) as used at
 * SM_call.py:353-363 (sigma (10,10) on the assembled field, (50,50) on the deltaU-change
 * weight) and Eval_dual_Dense_onlycil.py:366-367: mode 'reflect', truncate 4.  Host buffers
 * [ny, nx] float32, synchronous; in and out may alias.  Independent of the plan. */
int psm_gaussian_filter(psm_handle* h, const float* in, int32_t ny, int32_t nx, double sigma_y,
                        double sigma_x, float* out);

/* The same filter, and the whole tail of assemble_prediction (SM_call.py:352-363), on the device: in stream order, for a
 * case batch on the PLANNED grid, float32.
 *     result = gaussian_filter(field, sigma_field)                       if apply_filter
 *     w      = gaussian_filter(dU, sigma_weight)
 *     change = gaussian_filter((result - prev) * w, sigma_field);   next = prev + change   (pressureSM_Poisson, :843-848)
 * One launch per separable pass for the whole batch (csrc/psm_filter.hip): at most 4 launches with the weighting, 2 for a
 * filter alone.  Every output is the plain sum over its taps in a fixed order: case i of a batch is bit-identical to the same
 * field alone, and an output is NaN exactly where SciPy's is.
 * psm_bind_poststeps: sigma_field[2] / sigma_weight[2] = (sigma_y, sigma_x) of the two filters ((10,10) and (50,50) in the
 * reference).  Uploads the tap tables and reserves per-case scratch for max_cases cases: after it a step allocates nothing
 * and copies nothing.  PSM_ERR_ARG for a sigma that is not in (0, 1e4].  A psm_plan_grid or a model change drops the binding.
 * State errors (PSM_ERR_STATE) of the entries below: nothing bound, plan dropped after the bind, c_out != 1 with d_dU. */
int psm_bind_poststeps(psm_handle* h, const double* sigma_field, const double* sigma_weight);
int psm_unbind_poststeps(psm_handle* h);
/* d_in [n_cases,ny,nx,c_out] -> d_out, sigma_field on every channel; device pointers, asynchronous on `stream` (NULL: the
 * handle's); d_out may be d_in. */
int psm_filter_fields_device(psm_handle* h, const float* d_in, int32_t n_cases, float* d_out, void* stream);
/* The tail above on d_fields [n_cases,ny,nx] (c_out == 1): d_dU, d_prev [n_cases,ny,nx]; d_result receives the (filtered)
 * field and may be d_fields; d_change and d_next may each be NULL.  d_dU == NULL: filter only (apply_filter == 0: a copy),
 * any c_out. */
int psm_poststeps_device(psm_handle* h, const float* d_fields, int32_t n_cases, int32_t apply_filter, const float* d_dU,
                         const float* d_prev, float* d_result, float* d_change, float* d_next, void* stream);
/* psm_solve_grid_device + the tail in the same stream, as one graph replay; the solved field lives in a buffer of the handle. */
int psm_solve_poststeps_device(psm_handle* h, const float* d_grid, int32_t n_cases, const float* out_scale, int32_t apply_filter,
                               const float* d_dU, const float* d_prev, float* d_result, float* d_change, float* d_next, void* stream);
/* host buffers, synchronous; dU == NULL: filter only.  Like psm_solve_grid it solves again on the general path when the
 * bound-geometry guard trips. */
int psm_solve_poststeps(psm_handle* h, const float* grid, int32_t n_cases, const float* out_scale, int32_t apply_filter,
                        const float* dU, const float* prev, float* result, float* change, float* next);

/* The pressureSM_Poisson input features on the device, for a case batch on the PLANNED grid, and the whole time step behind
 * them: d_vel (Ux, Uy, dUx, dUy) -> features -> 4-channel deltas solve -> post-steps -> result / change / next, in device
 * memory from end to end.  Two launches for the whole batch (csrc/psm_features.hip): the arithmetic, its order and the
 * reduction partition are those of psm_poisson_features, so image i of a batch is bit-identical to that entry's on case i;
 * mean and standard deviation of the arcsinh transform are per case.
 * psm_bind_features: once per simulation, on the PLANNED grid; c_in == 4 and sdf_channel == 3, else PSM_ERR_STATE.
 * sdfunct [n_cases][ny*nx] float64 (raw SDF image, 0 in solids), k, max_abs[4] as in psm_poisson_features.
 * Uploads the SDF planes; reserves term / partial / image / staging buffers for n_cases cases and the pinned
 * slots for the per-step scalars: after it a step allocates nothing.  PSM_ERR_ARG: n_cases outside
 * [1, max_cases], a zero max_abs, non-finite k.  psm_plan_grid or a model change drops the binding.
 * The entries below take any n_cases in [1, bound count] (PSM_ERR_ARG otherwise); case i uses SDF slot i. */
int psm_bind_features(psm_handle* h, const double* sdfunct, int32_t n_cases, double k, const double* max_abs);
int psm_unbind_features(psm_handle* h);
/* d_vel [n_cases][4][ny*nx] float64 planes (ux, uy, dux, duy; dimensional, zero outside the flow, NaN allowed)
 * -> d_grid [n_cases,ny,nx,4] float32 (16-byte aligned).  LU: HOST array [n_cases][2] = (L, U) per case, copied
 * before the call returns (as out_scale is); PSM_ERR_ARG and nothing enqueued if any U == 0 or is not finite.
 * Device pointers, asynchronous on `stream` (NULL: the handle's). */
int psm_features_device(psm_handle* h, const double* d_vel, int32_t n_cases, const double* LU, float* d_grid, void* stream);
/* features + psm_solve_poststeps_device as ONE graph replay; the image lives in a buffer of the handle.  Needs
 * psm_bind_poststeps as well as psm_bind_features (PSM_ERR_STATE names the missing one).
 * d_dU == NULL: no weighting (then apply_filter == 0 is the plain solve, result = the assembled field). */
int psm_poisson_step_device(psm_handle* h, const double* d_vel, int32_t n_cases, const double* LU, const float* out_scale,
                            int32_t apply_filter, const float* d_dU, const float* d_prev,
                            float* d_result, float* d_change, float* d_next, void* stream);
/* host buffers, synchronous: vel [n_cases][4][ny*nx] float64 in, float32 fields out; one H2D of the velocities
 * (+ dU, prev), no image round trip.  Solves again on the general path after a guard trip, like psm_solve_poststeps. */
int psm_poisson_step(psm_handle* h, const double* vel, int32_t n_cases, const double* LU, const float* out_scale,
                     int32_t apply_filter, const float* dU, const float* prev, float* result, float* change, float* next);

/* Frames of cell columns on the single mesh of psm_set_geometry (its grid -> mesh tables are not needed), on the device: the
 * mesh -> grid step of psm_mesh_to_grid for n_frames arrays at once, every column into a plane of its own, and the Poisson
 * evaluator's whole frame behind it.  One launch for the batch (the frame is a launch dimension); statements, summation order,
 * `fill` and the 0 of a cell nobody writes are those of psm_mesh_to_grid, so a float64 plane holds the bits of that entry's
 * column and a float32 plane their plain cast (NaN stays NaN).  Every stored plane is written completely: no memset needed.
 * psm_bind_frames: after psm_set_geometry; n_frames in [1, max_cases], k in [1, 16] (PSM_ERR_ARG otherwise); PSM_ERR_STATE
 * without a mesh or on a case set (psm_set_geometry_cases).  Reserves the device and pinned staging the host entry goes
 * through (columns, extra planes, fields) for n_frames frames of k columns: after it a step allocates nothing.  A new mesh,
 * psm_plan_grid or a model change drops the binding. */
typedef struct { void* dst; int64_t frame_stride; int32_t as_f32; } psm_frame_col;   /* dst NULL: column not stored; stride in elements */
int psm_bind_frames(psm_handle* h, int32_t n_frames, int32_t k);
int psm_unbind_frames(psm_handle* h);
/* The stage alone.  d_cols [n_frames][n_cells][k] float64, row-major (per frame the array psm_mesh_to_grid takes); out: HOST
 * array [k], column c of frame f goes to out[c].dst + f * out[c].frame_stride + cell, as float64 or (as_f32) float32.  Device
 * pointers, asynchronous on `stream` (NULL: the handle's), nothing is copied: the descriptors travel in the launch.
 * PSM_ERR_ARG and nothing enqueued: k outside [1, 16], n_frames outside [1, bound count], a destination that is not aligned
 * to its element (8 / 4 bytes), a negative stride, every destination NULL. */
int psm_frames_to_grid_device(psm_handle* h, const double* d_cols, int32_t n_frames, int32_t k, int32_t fill,
                              const psm_frame_col* out, void* stream);
/* The Poisson evaluator's frames as ONE graph replay: planes -> psm_poisson_step_device, with fill = 1.  Columns 0-3 =
 * (Ux, Uy, dUx, dUy) go to the velocity planes of the feature binding; with weighting != 0 the last two columns (dU-change
 * weight, delta_p_prev) go as float32 to the post-steps' dU / prev buffers of the handle; the columns between go as float64 to
 * d_extra [n_frames][n_extra][ny*nx] (NULL: not stored).  k in [4, 16], with the weighting [6, 16].  weighting == 0: d_change
 * and d_next are not used.  Needs psm_bind_features, psm_bind_poststeps and psm_bind_frames (PSM_ERR_STATE names the missing
 * one); n_frames within every bound count.  LU [n_frames][2] and out_scale [n_frames] are HOST arrays copied before return. */
int psm_poisson_frames_device(psm_handle* h, const double* d_cols, int32_t n_frames, int32_t k, const double* LU,
                              const float* out_scale, int32_t apply_filter, int32_t weighting, double* d_extra,
                              float* d_result, float* d_change, float* d_next, void* stream);
/* host buffers, synchronous: one H2D of cols (k at most the bound count), D2H of the fields and (extra != NULL) of the extra
 * planes; no plane or image round trip.  Solves again on the general path after a guard trip, like psm_poisson_step. */
int psm_poisson_frames(psm_handle* h, const double* cols, int32_t n_frames, int32_t k, const double* LU,
                       const float* out_scale, int32_t apply_filter, int32_t weighting, double* extra,
                       float* result, float* change, float* next);

/* The per-frame error blocks of assembled fields on the device: what every evaluator of the reference prints per frame
 * (pressureSM_Poisson/SM_call.py:962-1043; SM_call.py:696-724) as eight float64 sums per (frame, pair), so that a metrics-only
 * sweep copies no field back.  raw[n_frames][n_pairs][8] = n, s1, s2 (count, sum, sum of squares of the non-NaN differences),
 * tmin, tmax (truth over the flow cells), pmin, pmax (non-NaN effective prediction), tnan (NaN truths on flow cells).  Per pixel:
 *     flow cell  iff  mask != 0 && mask == mask          (a NaN mask value is no flow: nan_to_num(sdfunct) / max_abs_dist == 0)
 *     truth    = plane, NaN -> 0 with truth_nan_to_zero
 *     pred_eff = (nan0(add) - nan0(sub)) + (double)pred  (add / sub: optional planes, ptr NULL = absent = 0)
 *     d        = pred_eff - truth;  a NaN d is left out of n, s1, s2
 * A plane is {ptr, frame_stride, elem_stride, as_f32}: pixel i of frame f is element ptr[f * frame_stride + i * elem_stride] of
 * float64 or (as_f32) float32 -- an [npix][c_out] field has elem_stride c_out.  Two launches (csrc/psm_mesh.hip), no atomics, one
 * fixed summation tree: raw is bit-reproducible from run to run; n = 0 leaves tmin = +inf, tmax = -inf.
 * psm_field_errors_device: the stage alone on a PLANNED handle (ny * nx pixels per plane), device pointers, plain launches,
 * asynchronous on `stream` (NULL: the handle's).  mask and pairs are HOST arrays that travel in the launch; the partial sums use
 * scratch of the plan (max_cases x PSM_ERR_MAX_PAIRS rows): a call allocates nothing, and calls on one handle must be ordered
 * by their streams.  PSM_ERR_ARG and nothing enqueued: a NULL or misaligned (8 / 4 bytes) mask, pred or truth plane, a misaligned
 * add / sub, n_pairs outside [1, PSM_ERR_MAX_PAIRS], n_frames outside [1, max_cases], a negative stride, d_raw not 8-byte aligned. */
#define PSM_ERR_MAX_PAIRS 4
typedef struct { const void* ptr; int64_t frame_stride; int64_t elem_stride; int32_t as_f32; } psm_err_plane;   /* strides in elements */
typedef struct { psm_err_plane pred, truth, add, sub; int32_t truth_nan_to_zero; } psm_err_pair;
int psm_field_errors_device(psm_handle* h, const psm_err_plane* mask, const psm_err_pair* pairs, int32_t n_pairs,
                            int32_t n_frames, double* d_raw, void* stream);
/* psm_poisson_frames_device (the same graph replay, unchanged) and the stage behind it on the same stream, with the Poisson
 * evaluator's three pairs, in this order: (next, nan0(extra 0)) = delta-p with the weighting, (result, nan0(extra 0)) = delta-p
 * without it, (next + nan0(extra 1) - nan0(extra 0), nan0(extra 1)) = p; extra 0 / 1 are the delta-p and p label columns, the mask
 * is the SDF plane of the feature binding.  d_raw [n_frames][3][8].  PSM_ERR_ARG and nothing enqueued: weighting == 0, k < 8 (no
 * two label columns), d_raw NULL or not 8-byte aligned, d_extra / d_result / d_next NULL; otherwise the errors of
 * psm_poisson_frames_device.  The device truth of delta-p is nan0(plane); the reference's nan_to_num(x / U^2) / m * m * U^2
 * differs from it by at most 4 ulp per element. */
int psm_poisson_frames_errors_device(psm_handle* h, const double* d_cols, int32_t n_frames, int32_t k, const double* LU,
                                     const float* out_scale, int32_t apply_filter, int32_t weighting, double* d_extra,
                                     float* d_result, float* d_change, float* d_next, double* d_raw, void* stream);
/* host buffers, synchronous: one H2D of cols, the step, the stage, and a D2H of n_frames * 3 * 8 doubles -- fields, change and
 * label planes stay in the handle's buffers.  Solves again on the general path after a guard trip, like psm_poisson_frames. */
int psm_poisson_frames_errors(psm_handle* h, const double* cols, int32_t n_frames, int32_t k, const double* LU,
                              const float* out_scale, int32_t apply_filter, int32_t weighting, double* raw);
/* Host arithmetic, no GPU and no handle: one raw row -> out[6] = normVal, biasNorm, stdeNorm, rmseNorm (percent), mean_err,
 * mean_sq_err, as the reference computes them from the arrays: norm = tmax - tmin, NaN when tnan > 0 (np.max of a truth with a
 * NaN); stde = sqrt(rmse^2 - bias^2), NaN when negative.  n == 0 (NumPy raises on the empty selection): out is all NaN, PSM_OK. */
int psm_error_metrics_from_sums(const double raw[8], double out[6]);

/* The frame batch of the pressureSM_deltas evaluator (SM_call.py:367-724) on the device: cell columns -> planes -> the solve's image,
 * label and truth planes -> solve (-> filter) -> the frame's two error blocks, without an image, a label or a field leaving the
 * device.  Columns of a frame: (dUx / U, dUy / U, dp / U^2, ...); columns beyond 2 are not stored.
 * psm_bind_deltas_frames: after psm_bind_frames, on a three-channel image with the SDF last and a one-channel field (c_in == 3,
 * sdf_channel == 2, c_out == 1; PSM_ERR_STATE otherwise, and without a frame binding).  sdfunct [ny*nx] float64 is the simulation's
 * raw SDF plane (NaNs allowed), max_abs = (max_abs_Ux, max_abs_Uy, max_abs_dist, max_abs_p), each finite and non-zero (PSM_ERR_ARG).
 * Keeps nan0(sdfunct) / max_abs_dist in float64 on the device -- channel 2 of every image, and the mask of the field errors (flow
 * cell iff != 0) -- and reserves image, label, truth, field, block partials, raw sums and pinned slots for the frame count bound
 * with psm_bind_frames: after it a step allocates nothing.  psm_bind_frames / psm_unbind_frames, a new mesh, psm_plan_grid or a
 * model change drop the binding. */
int psm_bind_deltas_frames(psm_handle* h, const double* sdfunct, const double* max_abs);
int psm_unbind_deltas_frames(psm_handle* h);
/* The image stage alone: psm_frames_to_grid_device (fill = 1) of columns 0-2 into the binding's planes, then one pack launch:
 *     d_grid  [n][ny][nx][3] float32 = (float)(nan0(v_c) / max_abs_c), c = 0, 1; channel 2 = (float)(nan0(sdfunct) / max_abs_dist)
 *     d_label [n][ny*nx]     float32 = (float)(nan0(v_2) / max_abs_p)                                  (NULL: not stored)
 *     d_truth [n][ny*nx]     float64 = (nan0(v_2) / max_abs_p) * max_abs_p * U2[f], left to right      (NULL: not stored)
 * -- divisions in float64, the cast behind them: the bits of the reference's NumPy statements (SM_call.py:439-445, :580).  U2
 * [n_frames] is a HOST array copied before return (may be NULL with d_truth NULL).  Device pointers aligned to their element,
 * asynchronous on `stream` (NULL: the handle's).  PSM_ERR_ARG and nothing enqueued: k outside [3, 16], n_frames outside [1, bound
 * count], d_cols or d_grid NULL, a misaligned destination, d_truth without U2. */
int psm_deltas_image_device(psm_handle* h, const double* d_cols, int32_t n_frames, int32_t k, const double* U2, float* d_grid,
                            float* d_label, double* d_truth, void* stream);
/* compute_in_block_error (utils.py:210-243; what psm_block_error gives for case 0 of the last solve) for n_frames frames on the
 * device: the decoded blocks of the LAST synchronous or device solve of at least n_frames cases on the handle's workspace (decoded
 * again from its network output, with its row scale) against the de-meaned label blocks of d_label [n][ny*nx] * row scale, over
 * the flow cells of d_grid [n][ny][nx][3] (SDF channel != 0).  d_raw [n_frames][8], 8-byte aligned: the sums of
 * psm_field_errors_device's layout, per frame the bits psm_block_error adds up on the host; psm_error_metrics_from_sums turns a row
 * into the metrics (mean_err / mean_sq_err = psm_block_error's out[0] / out[1]).  Three launches, no atomics, one fixed tree.
 * PSM_ERR_STATE: no deltas binding, no solve yet, the last solve ran on the ring, or it had fewer than n_frames cases. */
int psm_block_errors_device(psm_handle* h, const float* d_grid, const float* d_label, int32_t n_frames, double* d_raw, void* stream);
/* The whole step: planes -> image -> solve (-> the sigma_field filter of psm_bind_poststeps with apply_filter != 0; PSM_ERR_STATE
 * without that binding) as ONE graph replay.  Inside it the frames are solved one by one, each as the single case the evaluator's
 * per-frame call solves -- with a geometry bound for ONE case (psm_bind_geometry) the 6-launch route --, so a frame's field holds
 * the bits of psm_solve_grid on its image whatever the batch; every frame's network output is kept in the binding for the block
 * stage (psm_read_stage then shows the last frame's solve).  Then, with d_raw != NULL, plain launches on the same stream that leave
 * d_raw [n_frames][2][8]: row 0 = the (filtered) field against the truth plane over the cells with nan0(sdfunct) / max_abs_dist != 0
 * (psm_field_errors_device), row 1 = the blocks (psm_block_errors_device: always the unfiltered decoded blocks, as in the
 * reference).  d_result [n][ny*nx] float32 and d_truth [n][ny*nx] float64 may be NULL: the binding's buffers are used.  U2 and
 * out_scale [n_frames] are HOST arrays copied before return (out_scale NULL: 1).  k in [3, 16]. */
int psm_deltas_frames_device(psm_handle* h, const double* d_cols, int32_t n_frames, int32_t k, const double* U2,
                             const float* out_scale, int32_t apply_filter, float* d_result, double* d_truth, double* d_raw,
                             void* stream);
/* host buffers, synchronous: one H2D of cols (k at most the count bound with psm_bind_frames), D2H of what is non-NULL only --
 * result [n][ny*nx] float32, truth [n][ny*nx] float64, raw [n][2][8] (at least one of them).  Solves again on the general path
 * after a guard trip, like psm_poisson_frames. */
int psm_deltas_frames(psm_handle* h, const double* cols, int32_t n_frames, int32_t k, const double* U2, const float* out_scale,
                      int32_t apply_filter, float* result, double* truth, double* raw);

/* The frame batch of the U_to_gradP evaluator (Eval_dual_Dense_onlycil.py:418-687) on the device: cell columns -> planes -> the
 * solve's image and the three label planes -> solve (-> filter) -> integration into p -> the frame's four error blocks, without an
 * image, a label or a field leaving the device.  Columns of a frame: (Ux / U, Uy / U, dPdx (max_x - min_x) / U^2,
 * dPdy (max_y - min_y) / U^2, p / U^2, ...); columns beyond 4 are not stored.  No dimensional scale enters.
 * psm_bind_gradp_frames: after psm_bind_frames, on a three-channel image with the SDF last and a two-channel field (c_in == 3,
 * sdf_channel == 2, c_out == 2; PSM_ERR_STATE otherwise, and without a frame binding).  sdfunct [ny*nx] float64 is the simulation's
 * raw SDF plane (NaNs allowed), max_abs [5] the scales of grid channels 0-4, each finite and non-zero (PSM_ERR_ARG).  (center_y,
 * center_x), dx, dy: the cut and the spacings of psm_set_integration, fixed for the simulation; the tables are built once, into a set
 * of the binding's own, one geometry for every frame -- psm_bind_integration / psm_set_integration neither see nor change them, and
 * any frame count up to the bound one integrates.  PSM_ERR_UNSUPPORTED where the reference itself raises (see psm_set_integration);
 * then, as after every error, nothing is bound.  Keeps nan0(sdfunct) / max_abs[2] in float64 on the device -- channel 2 of every
 * image, and the mask of the field errors (flow cell iff != 0) -- and reserves planes, image, labels, gradient, p, raw sums and
 * pinned slots for the frame count bound with psm_bind_frames: after it a step allocates nothing.  psm_bind_frames /
 * psm_unbind_frames, a new mesh, psm_plan_grid or a model change drop the binding. */
int psm_bind_gradp_frames(psm_handle* h, const double* sdfunct, const double* max_abs, int32_t center_y, int32_t center_x, double dx,
                          double dy);
int psm_unbind_gradp_frames(psm_handle* h);
/* The image stage alone: psm_frames_to_grid_device (fill = 1) of columns 0-4 into the binding's planes, then one pack launch:
 *     d_grid  [n][ny][nx][3] float32 = ((float)(nan0(v_0) / max_abs_0), (float)(nan0(v_1) / max_abs_1), (float)(nan0(sdfunct) / max_abs_2))
 *     d_truth [n][3][ny*nx]  float64 = (nan0(v_2) / max_abs_3, nan0(v_3) / max_abs_4, nan0(v_4))             (NULL: not stored)
 * -- grid channels 3, 4 and 5 of the reference, the pressure label not divided (:463-467 loops over range(5)); divisions in float64,
 * the cast behind them: the bits of the reference's NumPy statements.  Device pointers aligned to their element, asynchronous on
 * `stream` (NULL: the handle's).  PSM_ERR_ARG and nothing enqueued: k outside [5, 16], n_frames outside [1, bound count], d_cols or
 * d_grid NULL, a misaligned destination. */
int psm_gradp_image_device(psm_handle* h, const double* d_cols, int32_t n_frames, int32_t k, float* d_grid, double* d_truth, void* stream);
/* The whole step as ONE graph replay: planes -> image and labels -> solve (-> the sigma_field filter of psm_bind_poststeps on both
 * gradient components with apply_filter != 0, in place of the unfiltered gradient; PSM_ERR_STATE without that binding) -> the two
 * integration launches for the batch with the binding's tables.  Inside it the frames are solved one by one, each as the single
 * case the evaluator's per-frame call solves -- with a geometry bound for ONE case (psm_bind_geometry) the 6-launch route --, so a
 * frame's gradient holds the bits of psm_solve_grid (psm_solve_poststeps) on its image whatever the batch, and its p the bits of
 * psm_integrate_gradp of that gradient (psm_read_stage then shows the last frame's solve).  Then, with d_raw != NULL, the two
 * launches of psm_field_errors_device on the same stream, over the cells with nan0(sdfunct) / max_abs_2 != 0, that leave d_raw
 * [n_frames][4][8]: row 0 = p against label plane 0 (the reference's own metric, :667-687: its "true" values are grid channel 3),
 * row 1 = p against label plane 2 (the pressure label), rows 2 and 3 = gradient components 0 and 1 against label planes 0 and 1.
 * d_gradp [n][ny*nx][2] float32 (8-byte aligned), d_p [n][ny*nx] float32 and d_truth [n][3][ny*nx] float64 may be NULL: the
 * binding's buffers are used.  out_scale [n_frames] is a HOST array copied before return (NULL: 1, what the evaluator passes).
 * PSM_ERR_ARG and nothing enqueued: k outside [5, 16], n_frames outside [1, bound count], d_cols NULL, a misaligned destination
 * (8 bytes for d_gradp, d_truth and d_raw, 4 for d_p). */
int psm_gradp_frames_device(psm_handle* h, const double* d_cols, int32_t n_frames, int32_t k, const float* out_scale,
                            int32_t apply_filter, float* d_gradp, float* d_p, double* d_truth, double* d_raw, void* stream);
/* host buffers, synchronous: one H2D of cols (k at most the count bound with psm_bind_frames), D2H of what is non-NULL only --
 * gradp [n][ny*nx][2] float32, p [n][ny*nx] float32, truth [n][3][ny*nx] float64, raw [n][4][8] (at least one of them).  Solves
 * again on the general path after a guard trip, like psm_deltas_frames. */
int psm_gradp_frames(psm_handle* h, const double* cols, int32_t n_frames, int32_t k, const float* out_scale, int32_t apply_filter,
                     float* gradp, float* p, double* truth, double* raw);

/* The frame batch of the two Chapter-4 evaluators (Chapter4/MLP/M_u/Evaluation/Eval_dual_Dense_onlycil.py: (Ux, Uy, SDF) -> p;
 * Chapter4/MLP/M_fU/Evaluation/Eval.py: (f(U), SDF) -> p) on the device: cell columns -> planes -> the solve's image and the truth
 * plane -> solve -> the frame's error block, without an image, a label or a field leaving the device.  Columns of a frame: the
 * c_in - 1 input channels (M_u: Ux / U, Uy / U; M_fU: f(U) / U^2), then the pressure label p / U^2; further columns are not stored.
 * No dimensional scale and no block stage enter: the reference compares prediction and label in normalised units (M_u :457-476).
 * psm_bind_chapter4_frames: after psm_bind_frames, on a PSM_VARIANT_CHAPTER5 handle with c_out == 1, c_in in {2, 3} and
 * sdf_channel == c_in - 1 (PSM_ERR_STATE naming the rule otherwise, and without a frame binding).  sdfunct [ny*nx] float64 is the
 * simulation's raw SDF image (0 in solids, NaNs allowed), max_abs [c_in + 1] the scales of the c_in - 1 input channels, of the
 * distance and of p, each finite and non-zero (PSM_ERR_ARG).  Keeps nan0(sdfunct) / max_abs_dist in float64 on the device -- channel
 * c_in - 1 of every image, and the mask of the field errors (flow cell iff != 0) -- and reserves planes, image, truth, field, raw
 * sums and pinned slots for the frame count bound with psm_bind_frames: after it a step allocates nothing.  psm_bind_frames /
 * psm_unbind_frames, a new mesh, psm_plan_grid or a model change drop the binding. */
int psm_bind_chapter4_frames(psm_handle* h, const double* sdfunct, const double* max_abs);
int psm_unbind_chapter4_frames(psm_handle* h);
/* The image stage alone: psm_frames_to_grid_device (fill = 1) of columns 0 .. c_in - 1 into the binding's planes, then one pack launch:
 *     d_grid  [n][ny][nx][c_in] float32 = (float)(nan0(v_c) / max_abs_c), c < c_in - 1; channel c_in - 1 = (float)(nan0(sdfunct) / max_abs_dist)
 *     d_truth [n][ny*nx]        float64 = nan0(v_{c_in - 1}) / max_abs_p                                     (NULL: not stored)
 * -- divisions in float64, the cast behind them: the bits of the reference's NumPy statements (M_u :215-225, M_fU :213-223).  Device
 * pointers aligned to their element, asynchronous on `stream` (NULL: the handle's).  PSM_ERR_ARG and nothing enqueued: k outside
 * [c_in, 16], n_frames outside [1, bound count], d_cols or d_grid NULL, a misaligned destination. */
int psm_chapter4_image_device(psm_handle* h, const double* d_cols, int32_t n_frames, int32_t k, float* d_grid, double* d_truth, void* stream);
/* The whole step as ONE graph replay: planes -> image and truth -> solve.  Inside it the frames are solved one by one, each as the
 * single case the evaluator's per-frame call solves -- with a geometry bound for ONE case (psm_bind_geometry) the 6-launch route --,
 * so a frame's field holds the bits of psm_solve_grid on its image whatever the batch (psm_read_stage then shows the last frame's
 * solve).  There is no filter: both reference files fail on their own filtered field (M_u :421, :457-458).  Then, with d_raw != NULL,
 * the two launches of psm_field_errors_device on the same stream, over the cells with nan0(sdfunct) / max_abs_dist != 0, that leave
 * d_raw [n_frames][1][8]: the field against the truth plane.  d_result [n][ny*nx] float32 and d_truth [n][ny*nx] float64 may be
 * NULL: the binding's buffers are used.  PSM_ERR_ARG and nothing enqueued: k outside [c_in, 16], n_frames outside [1, bound count],
 * d_cols NULL, a misaligned destination (4 bytes for d_result, 8 for d_truth and d_raw). */
int psm_chapter4_frames_device(psm_handle* h, const double* d_cols, int32_t n_frames, int32_t k, float* d_result, double* d_truth,
                               double* d_raw, void* stream);
/* host buffers, synchronous: one H2D of cols (k at most the count bound with psm_bind_frames), D2H of what is non-NULL only --
 * result [n][ny*nx] float32, truth [n][ny*nx] float64, raw [n][1][8] (at least one of them).  Solves again on the general path
 * after a guard trip, like psm_deltas_frames. */
int psm_chapter4_frames(psm_handle* h, const double* cols, int32_t n_frames, int32_t k, float* result, double* truth, double* raw);

/* A frame's dataset rows in, the per-frame scalars and the columns of the frame entries above made on the device: the head of the
 * three evaluators' timeSteps (surrogate.py) without per-cell host arithmetic, at half the bytes of the float64 columns.
 * rows [n_frames][n_cells][width] float32, row-major: the dataset frame cut at `indice`, nothing else done to it (r0, r1 = Ux, Uy;
 * r2 = p; r5, r6 = delta_U; r7 = delta_p; r8, r9 = delta_U_prev; r10 = delta_p_prev -- the gradP dataset: r6, r7 = dPdx, dPdy).
 * Two launches for the batch (csrc/psm_rows.hip; the frame is a launch dimension): partial maxima per (frame, 256-cell part), then a
 * finish launch in which every workgroup folds its frame's partials and writes its cells' columns.  All arithmetic is NumPy's on
 * float32, each operation rounded on its own (no fma), widened afterwards: U = max sqrt(r0^2 + r1^2), dU = max sqrt(r5^2 + r6^2),
 * c = max(|r5 - r8| + |r6 - r9|); a NaN anywhere makes a maximum NaN (np.max); U^2 = U * U in float32 (pow(U, 2.0) on a float32
 * wherever libm's powf rounds correctly; it is documented to within 1 ulp).  No atomics: the scalars are bit-reproducible.
 * `kind` selects the recipe; the columns d_cols [n_frames][n_cells][k] float64 hold the float32 results, widened:
 *   PSM_ROWS_DELTAS  k = 3: r5 / U, r6 / U, r7 / U^2
 *                    relevant = !(dU / U < 1e-4);  out-scale = (float)base * U^2 in float32
 *   PSM_ROWS_POISSON k = 8: r0, r1, r5, r6, r7, r2, (|r5 - r8| + |r6 - r9|) / c, r10
 *                    relevant = !(dU / U < 1e-4 || dU < 1e-6 || U < 1e-6) in float32;  out-scale = base * U^2 in float64
 *   PSM_ROWS_GRADP   k = 5: r0 / U, r1 / U, r6 * ex / U^2, r7 * ey / U^2, r2 / U^2, ex and ey rounded to float32 (what
 *                    EvaluationGradP holds);  relevant = 1;  out-scale = 1;  dU and c are not taken (0), nor is c for PSM_ROWS_DELTAS
 * d_scalars [n_frames][8] float64 = U, dU, c, relevant (1 / 0), U^2, out-scale, 0, 0.  A NaN maximum compares false: relevant.
 * An IRRELEVANT frame keeps its slot: all-zero columns, U = U^2 = 1, out-scale 0, relevant 0 (dU and c as measured); behind a
 * step its fields and sums are unspecified (they may be NaN), the other frames' bits are what they are without it, and it cannot
 * trip the bound-geometry guard -- the SDF channel comes from the binding.
 * psm_bind_rows: after psm_bind_frames; reserves device and pinned staging for the bound frame count x mesh cells x width rows,
 * the partial maxima and the scalar slots: after it a step allocates nothing.  width in [8, 16] (PSM_ERR_ARG).  Dropped by what
 * drops the frame binding (psm_bind_frames / psm_unbind_frames, a new mesh, psm_plan_grid, a model change). */
#define PSM_ROWS_DELTAS  0   /* pressureSM_deltas evaluator:  Evaluation.timeSteps */
#define PSM_ROWS_POISSON 1   /* pressureSM_Poisson evaluator: EvaluationPoisson.timeSteps */
#define PSM_ROWS_GRADP   2   /* U_to_gradP evaluator:         EvaluationGradP.timeSteps */
int psm_bind_rows(psm_handle* h, int32_t width);
int psm_unbind_rows(psm_handle* h);
/* The stage alone, as plain launches on device pointers, asynchronous on `stream` (NULL: the handle's).  n_cells in [1, cells of
 * the mesh]; params [4] = base, phi, ex, ey is a HOST array copied before return (base: PSM_ROWS_DELTAS / _POISSON; ex, ey:
 * PSM_ROWS_GRADP; phi is not used by the stage alone).  d_cols NULL: the frame binding's column buffer (it must have been bound with
 * at least k columns); d_scalars NULL: the binding's slots.  PSM_ERR_ARG and nothing enqueued: an unknown kind, width outside
 * [8, 16] (below 11 for PSM_ROWS_DELTAS / _POISSON), n_frames outside [1, bound count], n_cells outside the mesh, d_rows NULL, a
 * misaligned pointer (4 bytes for the rows, 8 for columns and scalars), a zero or non-finite base (kinds that use it), a
 * non-finite phi, ex or ey.  PSM_ERR_STATE names the missing binding. */
int psm_rows_prepare_device(psm_handle* h, int32_t kind, const float* d_rows, int32_t n_frames, int64_t n_cells, int32_t width,
                            const double* params, double* d_cols, double* d_scalars, void* stream);
/* The whole steps: the _frames entries of the same evaluator with the two launches at the head of their ONE graph replay.  rows +
 * width take the place of cols (the columns go through the frame binding's buffer, bound with at least k columns; the rows cover
 * the whole mesh), base (phi; ex, ey) the place of U2 / LU / out_scale: the finish launch writes the row scale of the decode, the
 * U^2 of the deltas pack and the (L, U) = (phi, U) of the feature launches into the device arrays those kernels read, so nothing but
 * the rows is uploaded in front of a step.  base = max_abs_p (deltas) / max_abs_delta_p (Poisson).  d_scalars [n_frames][8] beside
 * the other outputs (NULL: the binding's slots).  Every other argument, the bindings needed and the errors are those of the
 * counterpart (the Poisson entries pass k = 8) plus those of psm_rows_prepare_device; relevant frames hold the bits the counterpart
 * gives on the host-made columns and scalars. */
int psm_deltas_rows_device(psm_handle* h, const float* d_rows, int32_t n_frames, int32_t width, double base, int32_t apply_filter,
                           float* d_result, double* d_truth, double* d_raw, double* d_scalars, void* stream);
int psm_poisson_rows_device(psm_handle* h, const float* d_rows, int32_t n_frames, int32_t width, double base, double phi,
                            int32_t apply_filter, int32_t weighting, double* d_extra, float* d_result, float* d_change,
                            float* d_next, double* d_scalars, void* stream);
int psm_poisson_rows_errors_device(psm_handle* h, const float* d_rows, int32_t n_frames, int32_t width, double base, double phi,
                                   int32_t apply_filter, int32_t weighting, double* d_extra, float* d_result, float* d_change,
                                   float* d_next, double* d_raw, double* d_scalars, void* stream);
int psm_gradp_rows_device(psm_handle* h, const float* d_rows, int32_t n_frames, int32_t width, double ex, double ey,
                          int32_t apply_filter, float* d_gradp, float* d_p, double* d_truth, double* d_raw, double* d_scalars,
                          void* stream);
/* host buffers, synchronous: one H2D of the float32 rows (width at most the one bound with psm_bind_rows), D2H of what is non-NULL
 * only; scalars [n_frames][8] may be NULL.  They solve again on the general path after a guard trip, like their counterparts. */
int psm_deltas_rows(psm_handle* h, const float* rows, int32_t n_frames, int32_t width, double base, int32_t apply_filter,
                    float* result, double* truth, double* raw, double* scalars);
int psm_poisson_rows(psm_handle* h, const float* rows, int32_t n_frames, int32_t width, double base, double phi,
                     int32_t apply_filter, int32_t weighting, double* extra, float* result, float* change, float* next,
                     double* scalars);
int psm_poisson_rows_errors(psm_handle* h, const float* rows, int32_t n_frames, int32_t width, double base, double phi,
                            int32_t apply_filter, int32_t weighting, double* raw, double* scalars);
int psm_gradp_rows(psm_handle* h, const float* rows, int32_t n_frames, int32_t width, double ex, double ey, int32_t apply_filter,
                   float* gradp, float* p, double* truth, double* raw, double* scalars);

/* U_to_gradP: integrate the assembled (dp/dx, dp/dy) into p (integrate_field,
 * Eval_dual_Dense_onlycil.py:371-416, and the four-quadrant stitching :597-628).
 * psm_set_integration fixes the geometry: sdfunct [ny*nx] (self.sdfunct[:,:,0], also used by the
 * reference as the per-row "reset" index list), the cut (center_y = 200 and center_x of :599-600)
 * and the grid spacings np.diff(xl)[0], np.diff(yl)[0].  psm_integrate_gradp: gradp [ny,nx,2]
 * -> p [ny,nx], host float32 buffers, synchronous.  Returns PSM_ERR_UNSUPPORTED where the
 * reference itself raises (unequal flow-cell counts at the cut, index list outside a block). */
int psm_set_integration(psm_handle* h, int32_t ny, int32_t nx, const double* sdfunct, int32_t center_y,
                        int32_t center_x, double dx, double dy);
int psm_integrate_gradp(psm_handle* h, const float* gradp, float* p_out);

/* The same integration on the device, in stream order and for a case batch: the step that turns the gradP variant's
 * solve (psm_solve_grid_device leaves (dp/dx, dp/dy) in device memory) into a pressure without leaving the device.
 * Two launches for the whole batch (row scans of every case, then column scans + stitching means + the add).
 * psm_bind_integration: one integration geometry per case slot of the PLANNED grid (c_out == 2): sdfunct
 * [n_cases][ny*nx] float64, center_y / center_x [n_cases], spacings as psm_set_integration.  All-or-nothing:
 * PSM_ERR_UNSUPPORTED (the message names the case and the reason) where the reference itself raises for ANY case, and
 * then nothing is bound.  A psm_plan_grid or a model change drops the binding like it drops the geometry binding.
 * It is independent of psm_set_integration, whose single geometry of any size stays with the host entry above.
 * State errors (PSM_ERR_STATE): nothing bound, n_cases != the bound count, c_out != 2, plan dropped after the bind.
 * A NaN in the gradient reaches every p that is integrated through it; after a trip of the bound-geometry guard the
 * gradient is NaN everywhere and so is p (no special case; psm_synchronize reports the trip as for the solve). */
int psm_bind_integration(psm_handle* h, const double* sdfunct, int32_t n_cases,
                         const int32_t* center_y, const int32_t* center_x, double dx, double dy);
int psm_unbind_integration(psm_handle* h);
/* d_gradp [n_cases,ny,nx,2] (8-byte aligned) -> d_p [n_cases,ny,nx], device pointers, asynchronous on `stream`
 * (NULL: the handle's) */
int psm_integrate_gradp_device(psm_handle* h, const float* d_gradp, int32_t n_cases, float* d_p, void* stream);
/* psm_solve_grid_device + the integration in the same stream.  d_gradp may be NULL (the gradient then lives in a
 * buffer of the handle) or receive the assembled gradient as psm_solve_grid_device would have written it. */
int psm_solve_pressure_device(psm_handle* h, const float* d_grid, int32_t n_cases, const float* out_scale,
                              float* d_gradp, float* d_p, void* stream);
/* host buffers, synchronous: grid [n_cases,ny,nx,c_in] -> p [n_cases,ny,nx] (one H2D, one D2H of half the size).
 * Like psm_solve_grid it solves again on the general path when the bound-geometry guard trips. */
int psm_solve_pressure(psm_handle* h, const float* grid, int32_t n_cases, const float* out_scale, float* p);

/* Wait for everything submitted through this handle. */
int psm_synchronize(psm_handle* h);

/* ---- introspection ------------------------------------------------------- */
/* Copy an intermediate of the LAST solve to host memory (float32).  PSM_ERR_STATE when that solve did not leave it: it ran
 * on a ring slot's workspace (psm_submit_grid*, psm_ring_submit), or, for PSM_STAGE_BLOCK_PRED, on the geometry-bound path,
 * which never stores the decoded blocks. */
int psm_read_stage(psm_handle* h, int32_t stage, float* dst, size_t dst_floats);
/* Run one solve with a HIP event pair around every kernel group on the
 * launch stream; ms[PSM_K_COUNT] receives the durations in milliseconds. */
int psm_profile_solve(psm_handle* h, const float* d_grid, int32_t n_cases,
                      float* d_fields, float* ms);
/* Accumulated device time (ms) and launch count of kernel group `k`, measured
 * with HIP events on the launch stream while event timing is enabled.
 * on = 0 disables; on = R >= 1 launches the (idempotent) group R times back to
 * back between the two events of every solve, which amortises the ~2.7 us an
 * event pair adds to a single launch. */
int psm_enable_kernel_timing(psm_handle* h, int32_t kernel, int32_t on);
int psm_get_kernel_timing(psm_handle* h, int32_t kernel, double* total_ms, int64_t* launches);

/* ---- the Poisson-model step at the solver boundary: cells [n,5] -> p [n], two-frame state on the device ----------------------
 * pressureSM_Poisson's timeStep behind the contract of psm_solve (pressureSM_Poisson/SM_call.py:815-818: "This only needs to be done
 * when calling the SM in the CFD solver").  Call k passes cells_k = (Ux, Uy, Cx, Cy, p(t-1)); the handle keeps, per mesh cell,
 * u_prev = U of the previous call, du_prev = its dU and p_prev = its column 4, and a count of held frames (0, 1 or 2).
 * One step, all of it float64 per cell and rounded operation by operation:
 *   head   U = max sqrt(Ux^2 + Uy^2) (SMP:556); dU = cells[:,0:2] - u_prev; c_cell = |dUx - du_prev_x| + |dUy - du_prev_y| (SMP:549),
 *          c = max c_cell, weight = c_cell / c (0 where c == 0; SMP:550); dp_prev = cells[:,4] - p_prev.  No atomics: bit-reproducible.
 *   mesh -> grid   interpolate_fill + last-writer scatter, the statements of psm_mesh_to_grid: (Ux, Uy, dUx, dUy) as float64 into the
 *          feature binding's velocity planes (NaNs kept), weight and dp_prev as float32 into the post-steps' dU / prev planes with
 *          NaN -> 0: a solver's tables carry negative weights (PM:210, no IDW fallback), and a NaN there would reach every pixel within
 *          the sigma_weight filter's radius.
 *   chain  psm_poisson_step_device's launches; (L, U) = (phi, U) and the decode's row scale max_abs_delta_p * U^2 are written on the
 *          device by the head.  Nothing but `cells` is uploaded in front of a step.
 *   tail   field = next = prev + change with the weighting, else result (SMP:842-847), already dimensional;
 *          dp[n] = sum_j field[cell_of_point[vtx[n][j]]] * wts[n][j]; p_out[n] = cells[n][4] + dp[n], and cells[n][4] bit for bit where
 *          psm_solve falls back (near-wall cell, negative weight, NaN: PM:494-496).  The same thread then turns the state over:
 *          du_prev := cells[:,0:2] - u_prev, u_prev := cells[:,0:2], p_prev := cells[:,4].
 * Head and tail are three launches in the chain's graph replay.  A step is SKIPPED when !(U > 0 and finite), or with the weighting
 * when c is NaN: the chain runs on U = 1, out-scale 0 and all-zero columns, p_out = cells[:,4], the state still turns over.  The
 * evaluator's "irrelevant time step" rule (SMP:562-567) is not applied, as in psm_solve_delta.  A step needs 1 + weighting held
 * frames; with fewer it is a PRIMING step: PSM_OK, p_out = cells[:,4] bit for bit, the frame is pushed (one launch, no network),
 * `steps` is not incremented.  A push at 0 frames sets du_prev := 0.
 * psm_bind_poisson_solve: needs the single mesh of psm_set_geometry with its grid -> mesh tables (PSM_ERR_ARG without them; a case set:
 * PSM_ERR_STATE), c_in == 4, c_out == 1, sdf_channel == 3 (PSM_ERR_UNSUPPORTED) and psm_bind_features, psm_bind_poststeps and
 * psm_bind_frames (k >= 6) (PSM_ERR_STATE names the missing one); phi and max_abs_delta_p finite and non-zero (PSM_ERR_ARG).  It
 * allocates the state, the partial maxima and the scalar slots: after it a step allocates nothing.  Whatever drops one of the three
 * bindings or the mesh drops it; psm_poisson_solve_state then reports 0 frames.
 * psm_poisson_solve_push: one frame from the host (a restart primes with two); _reset: frames = 0, steps = 0; _state: either may be NULL.
 * psm_solve_poisson: host buffers, synchronous: one H2D copy of cells and one D2H copy of p through the handle's pinned staging, or
 * straight from / into ranges registered with psm_host_register.  One step in flight per handle across all step kinds.
 * psm_solve_poisson_device: device pointers, 8-byte aligned, asynchronous on `stream` (NULL: the handle's), copies nothing.
 * d_fields [3][ny*nx] float32 receives (result, change, next) and may be NULL; change / next are written only with the weighting.
 * d_scalars [8] float64 = U, c, U^2, out-scale, skip, frames held before the call, 0, 0; NULL: the binding's slots.
 * Not provided: _begin / _end halves and the psm_pin_buffers direct routes; case sets: the `_cases` entries below. */
int psm_bind_poisson_solve(psm_handle* h, double phi, double max_abs_delta_p, int32_t weighting, int32_t apply_filter);
int psm_unbind_poisson_solve(psm_handle* h);
int psm_poisson_solve_push(psm_handle* h, const double* cells, int64_t n);
int psm_poisson_solve_reset(psm_handle* h);
int psm_poisson_solve_state(const psm_handle* h, int32_t* frames, int64_t* steps);
int psm_solve_poisson(psm_handle* h, const double* cells, int64_t n, int32_t rank, double* p_out);
int psm_solve_poisson_device(psm_handle* h, const double* d_cells, double* d_p, float* d_fields, double* d_scalars, void* stream);
/* The same step for the case set of psm_set_geometry_cases under the four-channel model: K meshes on one grid advanced by ONE call,
 * the chain run on K cases between the three mesh-end launches in their case-batched form (the case is launch dimension y), in one
 * graph replay.  Cell-side arrays are the cases' concatenated in case order, as for psm_solve_cases: cells [sum n_i, 5], p [sum n_i].
 * Per case the semantics are those above, bit for bit what psm_solve_poisson gives on a single mesh with the same tables: U, c, the
 * weight, dp_prev, the fallback cells, the turn-over of the state.  Every case decides on its own whether its step is SKIPPED (its
 * chain runs on U = 1, out-scale 0 and zero columns, it returns cells[:,4] and scalars[k][4] == 1; its neighbours are not
 * affected).  The set has ONE frame counter and one step counter: all cases are pushed and advanced together; a priming step returns
 * p = cells[:,4] for every case.  No atomics: a step is bit-reproducible.
 * psm_bind_poisson_solve_cases: needs a case set (PSM_ERR_STATE; on a single mesh the message names psm_bind_poisson_solve), c_in == 4,
 * c_out == 1, sdf_channel == 3 (PSM_ERR_UNSUPPORTED), psm_bind_features for at least the set's K cases, with the K sdfuncts in case
 * order, and psm_bind_poststeps (PSM_ERR_STATE names the missing one, or says that the features are bound for fewer cases); phi and
 * max_abs_delta_p finite and non-zero (PSM_ERR_ARG).  psm_bind_frames is not needed (it belongs to the single mesh).  It allocates the
 * state (zeroed), the partial maxima and the scalar slots: after it a step allocates nothing.  Whatever drops the case set, the
 * features or the post-steps drops it.  psm_poisson_solve_reset, psm_poisson_solve_state and psm_unbind_poisson_solve serve whichever
 * of the two bindings the handle holds; psm_solve_poisson* and psm_poisson_solve_push on this binding, and the entries below on
 * psm_bind_poisson_solve's, are PSM_ERR_STATE naming the other form.
 * psm_solve_cases_poisson_device: d_fields [3][K][ny*nx] float32 receives (result, change, next) and may be NULL; d_scalars [K][8]
 * float64, one row per case as above, NULL: the binding's slots; pointers aligned as for psm_solve_poisson_device, checked before
 * anything is enqueued.
 * Not provided either: _begin / _end halves and the psm_pin_buffers direct routes. */
int psm_bind_poisson_solve_cases(psm_handle* h, double phi, double max_abs_delta_p, int32_t weighting, int32_t apply_filter);
int psm_poisson_solve_push_cases(psm_handle* h, const double* cells);                 /* [sum n_i, 5] */
int psm_solve_cases_poisson(psm_handle* h, const double* cells, double* p_out);       /* [sum n_i, 5] -> [sum n_i] */
int psm_solve_cases_poisson_device(psm_handle* h, const double* d_cells, double* d_p, float* d_fields, double* d_scalars, void* stream);

/* ---- the gradient-model step at the solver boundary: cells [n,5] -> p [n] through U -> grad p -> p, no state -------------------
 * The U_to_gradP model behind the contract of psm_solve, on a PSM_VARIANT_GRADP handle with c_in == 3, c_out == 2, sdf_channel == 2
 * (psm_solve* itself keeps refusing c_out == 2).  cells = (Ux, Uy, Cx, Cy, p(t-1)) float64 in, p float64 out.  One step:
 *   head   psm_solve's two launches as they are: U = max sqrt(Ux^2 + Uy^2), then mesh -> grid.  `maxs` of the geometry call is read
 *          as (max_abs_Ux, max_abs_Uy, max_abs_dist, unused); the model's convention is normalise_sdf = 1, fill_input = 1
 *          (Eval_dual_Dense_onlycil.py:447-451, :466), passed by the caller to psm_set_geometry* as for the delta step.
 *   solve  the route psm_set_geometry* bound for the mesh, without a row scale: the gradient stays in the network's normalised units.
 *   filter with apply_filter, the sigma_field filter of psm_bind_poststeps on both components, as in psm_gradp_frames_device.
 *   integration  the two launches of psm_integrate_gradp_device on tables of the binding's own, built from the raw sdfunct given to
 *          psm_set_geometry* (the handle keeps a float64 host copy) and the caller's cut, with the spacings
 *          sx = dx * max_abs_dPdx / extent_x and sy = dy * max_abs_dPdy / extent_y (:537-538, the inverse of :441-442 and :467-468).
 *          The integration is linear in (SdPx dx, SdPy dy), so the float32 plane q [ny][nx] it leaves is p / U^2.
 *   tail   reference PSM_GRADP_REF_OUTLET: s = mean_y(3 q[y][nx-1] - q[y][nx-2]) / 3 (the outlet rule of python_module.py:472 /
 *          SM_call.py:350 on the integrated plane; p = 0 at the outlet), in float64 over all ny rows, recomputed by every workgroup in
 *          one fixed tree: no atomics, a step is bit-reproducible.  PSM_GRADP_REF_NONE: s = 0.0 exactly.  Per mesh cell n, every
 *          operation rounded on its own: acc = sum_j ((double)q[cell_of_point[vtx[n][j]]] - s) * wts[n][j] for j = 0, 1, 2 in order,
 *          p = acc * (U * U); p_out[n] = p, or cells[n][4] bit for bit where psm_solve falls back (near-wall cell, negative weight,
 *          NaN acc: PM:494-496).  A NaN in q's last two columns makes s NaN: every cell then keeps its previous p.
 * The whole step is one graph replay: two head launches, the solve, optionally two filter launches, two integration launches, one
 * tail launch.  There is no state, no priming step and no skip rule: U enters as it does in psm_solve.
 * psm_bind_gradp_solve: needs the gradP handle (PSM_ERR_UNSUPPORTED otherwise), the single mesh of psm_set_geometry (PSM_ERR_STATE; on
 * a case set the message names psm_bind_gradp_solve_cases) with its grid -> mesh tables (PSM_ERR_ARG without them) and, with
 * apply_filter, psm_bind_poststeps (PSM_ERR_STATE naming it); dx, dy, extent_x, extent_y and max_abs_grad = (max_abs_dPdx, max_abs_dPdy)
 * finite and non-zero and a known `reference` (PSM_ERR_ARG); a cut the reference itself cannot process is PSM_ERR_UNSUPPORTED with the
 * message of psm_bind_integration (a cut outside the grid: PSM_ERR_ARG).  All-or-nothing: it allocates the integration tables, the
 * image, the gradient, the q plane and the scalar slots; after it a step allocates nothing.  Whatever drops the mesh, the plan, the
 * model or, with apply_filter, the post-steps drops it.
 * psm_solve_gradp: host buffers, synchronous: one H2D copy of cells and one D2H copy of p through the handle's pinned staging, or
 * straight from / into ranges registered with psm_host_register.  One step in flight per handle across all step kinds.
 * psm_solve_gradp_device: device pointers, asynchronous on `stream` (NULL: the handle's), copies nothing.  Optional outputs, any of
 * them NULL: d_image [ny][nx][3] float32, the image that was solved; d_gradp [ny][nx][2] float32, the gradient behind the filter;
 * d_pgrid [ny][nx] float32, q before the shift; d_scalars [8] float64 = U, U^2, s, sx, sy, 0, 0, 0 (NULL: the binding's slots).
 * Alignment (8 bytes for cells, p, d_gradp and d_scalars, 4 for d_image and d_pgrid) is checked before anything is enqueued.
 * Not provided: _begin / _end halves and the psm_pin_buffers direct routes.
 * The `_cases` entries are the same step for the case set of psm_set_geometry_cases, which accepts the gradP model for them alone
 * (psm_solve_cases* and the delta entries on such a set stay PSM_ERR_UNSUPPORTED): K meshes advanced by ONE graph replay, the case is
 * launch dimension y of the mesh ends.  center_y / center_x [K] are the cuts in case order (an unprocessable one is named "case k: ");
 * cells [sum n_i, 5], p [sum n_i], d_image [K][ny][nx][3], d_gradp [K][ny][nx][2], d_pgrid [K][ny][nx], d_scalars [K][8].  For case k
 * every bit of p, q and s is what psm_solve_gradp gives on a handle holding that case's tables alone.  Each form's step entries
 * refuse the other's binding by name (PSM_ERR_STATE); psm_unbind_gradp_solve serves whichever of the two is held. */
#define PSM_GRADP_REF_NONE   0
#define PSM_GRADP_REF_OUTLET 1
int psm_bind_gradp_solve(psm_handle* h, int32_t center_y, int32_t center_x, double dx, double dy, double extent_x, double extent_y,
                         const double* max_abs_grad /* [2]: dPdx, dPdy */, int32_t apply_filter, int32_t reference);
int psm_bind_gradp_solve_cases(psm_handle* h, const int32_t* center_y, const int32_t* center_x, double dx, double dy, double extent_x,
                               double extent_y, const double* max_abs_grad, int32_t apply_filter, int32_t reference);
int psm_unbind_gradp_solve(psm_handle* h);
int psm_solve_gradp(psm_handle* h, const double* cells, int64_t n, int32_t rank, double* p_out);
int psm_solve_gradp_device(psm_handle* h, const double* d_cells, double* d_p, float* d_image, float* d_gradp, float* d_pgrid,
                           double* d_scalars, void* stream);
int psm_solve_cases_gradp(psm_handle* h, const double* cells, double* p_out);         /* [sum n_i, 5] -> [sum n_i] */
int psm_solve_cases_gradp_device(psm_handle* h, const double* d_cells, double* d_p, float* d_image, float* d_gradp, float* d_pgrid,
                                 double* d_scalars, void* stream);

/* ---- input trust: can the model represent the image the last solve ran on? ----
 * The network sees nothing but the p_in PCA coefficients of every input block; a block far outside the span of the retained
 * components gives coefficients, and a p, that mean nothing, and no other entry says so.  For block row m = case * B + b of the
 * LAST solve on the handle's own workspace, with x the block's S*S*c_in float32 image values in the column order of comp_in
 * ([r][c][ch]), mu = (float)mean_in, C = (float)comp_in[:p_in], G = C C^T in float64 and z the coefficients the encode of that solve
 * produced -- PSM_STAGE_X_INPUT with the model's input scaler undone in float64, z_p = (xin[m][p] - ib[p]) / ia[p]:
 *     n   = sum_k (x_k - mu_k)^2
 *     spe = n - 2 sum_p z_p^2 + z^T G z        ( = |x - mu - C^T z|^2 at z = C (x - mu), for any C, orthonormal or not: the SPE / Q
 *                                                statistic; the encode's float32 rounding of z moves spe / n by 1e-10 .. 5e-7 )
 * two float64 per block row, out[(case * B + b) * 2 + {0, 1}].  Nothing is clamped (a spe slightly below zero is rounding); n == 0
 * gives spe = 0.  1 - spe / n is the explained share, comparable with the var_in the model's input PCA was cut at; the caller forms
 * it, and decides what a low value means for its step.  Float64 sums, no atomics, one fixed tree: the same solve gives the same bits.
 * psm_bind_trust: once per model + plan, behind psm_plan_grid.  comp_in [p_in][K_in] is the array psm_set_pca was given; the Gram
 * matrix is built on the device from a float32 copy that is released before the call returns; after it the entries below allocate
 * nothing.  PSM_ERR_UNSUPPORTED on a bf16 handle (its encode rounds the inputs), PSM_ERR_ARG when a factor of the input scaler is
 * zero or not finite in float32.  psm_plan_grid and the model setters drop the binding.
 * psm_trust_last_device: two launches on `stream` (NULL: the handle's), asynchronous, d_out [n_cases][B][2] float64 in device
 * memory.  The scored solve is whatever chain ran last: psm_solve_grid*, every step at the solver boundary (psm_solve*,
 * psm_solve_cases*, the delta, Poisson and gradient steps; of a priming or skipped step, the chain before it) with n_cases the
 * solve's; an evaluator's frame step solves its frames one by one, so it leaves its last frame, n_cases = 1.  The image must still be
 * there unchanged: the library's own images are (a released one is PSM_ERR_STATE), the d_grid of psm_solve_grid_device and of the
 * *_device step entries is the caller's to keep.  The launches are ordered on `stream` only: give the solve's stream.
 * psm_trust_last: the same through the binding's staging, synchronous; *n_cases (may be NULL) receives the scored solve's case
 * count, out_doubles is the capacity of `out` (>= n_cases * B * 2, else PSM_ERR_ARG).
 * PSM_ERR_STATE, nothing enqueued: not bound, not planned, no solve since the plan, or the last solve ran on a ring slot's workspace
 * (the rule of psm_block_error).  No entry here is part of any solve's launch sequence, and none changes a bit of a field. */
int psm_bind_trust(psm_handle* h, const double* comp_in);
int psm_unbind_trust(psm_handle* h);
int psm_trust_last_device(psm_handle* h, double* d_out, void* stream);
int psm_trust_last(psm_handle* h, int32_t* n_cases, double* out, size_t out_doubles);

/* Dispatch-level time of EVERY kernel of the solve path: `steps` solves of d_grid through the launch sequence of
 * psm_solve_grid_device on the handle's stream, each dispatch stamped with its own begin / end by
 * hipExtLaunchKernelGGL (the timestamps rocprofv3 --kernel-trace reads).  names [cap][64] receives the kernel
 * names in first-launch order, total_ms / launches [cap] their accumulated duration and dispatch count,
 * *n_kernels the number of distinct kernels (may exceed cap).  While an integration is bound for n_cases cases
 * (psm_bind_integration) the timed step is that of psm_solve_pressure_device: its two launches are stamped too; while
 * post-steps are bound on a c_out == 1 handle (psm_bind_poststeps), that of psm_solve_poststeps_device with the weighting
 * and apply_filter (dU and prev: the handle's scratch); with the Poisson features bound for n_cases cases as well
 * (psm_bind_features), that of psm_poisson_step_device: the two feature launches write the handle's image from its staging
 * planes and the solve reads that image, not d_grid. */
int psm_time_kernels(psm_handle* h, const float* d_grid, int32_t n_cases, float* d_fields, int32_t steps, char* names,
                     double* total_ms, int64_t* launches, int32_t cap, int32_t* n_kernels);
/* The same pass, reported per kernel as the MEDIAN and the 10th / 90th percentile of its dispatch durations in microseconds
 * (p10_us / p90_us may be NULL): one slow dispatch moves a mean of a few hundred samples, not these.  bench.py's roofline uses it. */
int psm_time_kernels_q(psm_handle* h, const float* d_grid, int32_t n_cases, float* d_fields, int32_t steps, char* names,
                       double* median_us, double* p10_us, double* p90_us, int64_t* launches, int32_t cap, int32_t* n_kernels);
/* Host-buffer throughput measured from a C++ loop on the calling thread (no per-call binding overhead), through the
 * public entries only: `steps` solves of the `n_inputs` host grids [n_inputs][n_cases, ny, nx, c_in] in rotation after
 * `warmup` untimed ones; *seconds = wall time of the timed solves (steady_clock, first submission to last result).
 *   mode 0  psm_solve_grid, pageable caller memory (the synchronous py_func contract)
 *   mode 1  psm_submit_grid / psm_wait_grid ring, pageable caller memory, `depth` tickets in flight
 *   mode 2  psm_submit_grid_io ring on caller-registered memory (grids and result buffers registered for the run)
 *   mode 3  psm_ring_acquire / submit / wait: the slots' pinned buffers hold the inputs (packed before the timed
 *           region, like a solver that writes its fields straight into the slot), results are left in the slots
 * last_fields (optional) receives the result of the last solve [n_cases, ny, nx, c_out]. */
int psm_bench_host(psm_handle* h, const float* grids, int32_t n_inputs, int32_t n_cases, int32_t mode, int32_t depth,
                   int32_t steps, int32_t warmup, double* seconds, float* last_fields);

/* Median elapsed time (ms) of `n` EMPTY HIP event pairs recorded back to back on the launch
 * stream: the cost of the event timing itself, to be subtracted from per-launch event times. */
int psm_event_pair_overhead(psm_handle* h, int32_t n, double* median_ms);

/* ---- host-only helpers (no GPU needed) ----------------------------------- */
/* Block layout of a variant: writes up to `cap` rows of (y0, x0, idx_i, idx_j)
 * into blocks[4*cap]; returns the number of blocks (or <0).  n_x / n_y as at
 * PM:306-307, SMD:461-462, UGP:479-480. */
int psm_layout(int32_t variant, int32_t ny, int32_t nx, int32_t block, int32_t overlap,
               int32_t* blocks, int32_t cap, int32_t* n_x, int32_t* n_y);
/* Which block (index into the layout) supplies each output cell after all
 * pastes, and from which local cell: owner[ny*nx] = b*S*S + r*S + c (or -1). */
int psm_owner_map(int32_t variant, int32_t ny, int32_t nx, int32_t block, int32_t overlap,
                  int32_t strict_degenerate, int32_t* owner);
/* Host replay of the device reassembly (strip table -> offset chain -> owner-map
 * paste) on caller-supplied decoded blocks pred[B, S*S*c_out] and one grid
 * [ny, nx, c_in].  Verification helper for the plan tables; never called by
 * psm_solve_*.  offsets [c_out, B] and shifts [c_out] may be NULL. */
int psm_debug_reassemble_host(int32_t variant, int32_t ny, int32_t nx, int32_t block, int32_t overlap,
                              int32_t strict_degenerate, int32_t c_in, int32_t c_out, int32_t sdf_channel,
                              const float* grid, const float* pred, float* fields, float* offsets,
                              float* shifts);
/* Diagnostic: with PSM_GUARD_PAGES=1 in the environment (read once, at the first allocation) every device buffer of the
 * library is placed at the end of its own mapping with an unmapped granule behind it, so that a kernel running past the end
 * of a buffer takes a GPU page fault instead of touching a neighbour (the GPU address sanitizer's stand-in for that class;
 * csrc/psm_alloc.cpp).  psm_debug_guard_pages: 1 when the mode is on; psm_debug_malloc / psm_debug_free: the same allocator
 * for a caller's own test buffers (hipError_t values). */
int psm_debug_guard_pages(void);
int psm_debug_malloc(void** ptr, size_t bytes);
int psm_debug_free(void* ptr);
/* Synchronous copies between device memory and ordinary (pageable) host memory through the library's pinned bounce buffer --
 * what every entry of this library that takes host pointers does internally (the GPU never touches caller memory that was
 * not registered explicitly; csrc/psm_alloc.h says why).  For a caller's own test buffers; hipError_t values. */
int psm_debug_copy_to_device(void* dst_device, const void* src_host, size_t bytes);
int psm_debug_copy_to_host(void* dst_host, const void* src_device, size_t bytes);
int psm_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* PSM_H_ */
