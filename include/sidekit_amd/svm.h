/* sidekit_amd/svm.h -- the GMM-supervector SVM back end (sidekit/svm_training.py): M independent two-class C-SVC duals over one shared
 * background Gram block, solved in one launch.  One entry point of libsidekit_amd.so under the conventions of mixture.h (error classes,
 * device pointers, the stream argument), in a header of its own and bound by a table of its own (sidekit_amd/_lib.py SVM_SIGNATURES):
 * the other headers and their tables are pinned symbol for symbol.  The entry point needs none of the sc_* workspace: everything a
 * model's solver keeps between iterations lives in the LDS of its workgroup. */
#ifndef SIDEKIT_AMD_SVM_H
#define SIDEKIT_AMD_SVM_H
#include "mixture.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A workgroup keeps three doubles per point in LDS (the dual variable a, the gradient G and the kernel's diagonal) and
 * SC_SVM_LDS_RESERVED bytes for its reductions.  A single workgroup may declare all 160 KiB of a CU's LDS, which bounds the points of
 * one problem: (163840 - 1024) / 24 = 6784. */
#define SC_SVM_LDS_BYTES 163840
#define SC_SVM_LDS_RESERVED 1024
#define SC_SVM_MAX_N ((SC_SVM_LDS_BYTES - SC_SVM_LDS_RESERVED) / 24)

/* d_status[m] */
#define SC_SVM_CONVERGED 0     /* the gap fell below eps */
#define SC_SVM_MAX_ITER 1      /* max_iter updates were made and the gap is still >= eps: the model holds what it has (libsvm's behaviour) */
#define SC_SVM_BAD_OFFSETS 2   /* d_en_off / d_ee_off of this model do not describe rows inside the arrays: nothing else is written for it */

/* Model m's problem has n_m = B + csn_m points: the B background rows, then its csn_m = d_en_off[m + 1] - d_en_off[m] enrolment rows
 * (rows d_en_off[m] .. of K_eb).  y = +1 on the background (libsvm's positive class is the first label it meets, the reference lists the
 * background first) and y = -1 on the targets.  It solves
 *     min_a  1/2 a' Q a - e' a     subject to  0 <= a_i <= C_m,  y' a = 0,      Q_ij = y_i y_j K_ij,
 * in float64 with libsvm's solver without shrinking:
 *   - working-set selection WSS2 (Fan, Chen and Lin 2005): i maximises -y_t G_t over I_up = {y_t = +1, a_t < C} u {y_t = -1, a_t > 0};
 *     j minimises -(g_t)^2 / q_t over the t of I_low = {y_t = +1, a_t > 0} u {y_t = -1, a_t < C} with g_t = -y_i G_i + y_t G_t > 0,
 *     q_t = K_ii + K_tt - 2 K_it, and q_t = tau = 1e-12 where that curvature is not positive;
 *   - libsvm's two clipped pair updates (y_i != y_j and y_i == y_j) and G_k += Q_ik da_i + Q_jk da_j from the two kernel rows;
 *   - it stops when gap = max_{I_up}(-y G) - min_{I_low}(-y G) < eps, or when no t qualifies for j, or after max_iter updates;
 *   - rho = the mean of y_i G_i over the free variables (0 < a_i < C); with no free variable, the midpoint of
 *     ub = min(y G over {a = C, y = -1} u {a = 0, y = +1}) and lb = max(y G over {a = C, y = +1} u {a = 0, y = -1}).
 * THE TIE RULE: both selections take, among candidates of equal value, the LARGEST index (libsvm's `>=` and `<=` in an ascending
 * scan).  Ties occur: in the first iteration every background point ties.  Reductions carry (value, index) pairs, so the rule does not
 * depend on how the points are spread over lanes.
 * A point's kernel row is read as stored: K_bb[i][.] and K_eb[.][i] for a background point i, K_eb[r][.] and K_ee_m[r][.] for target r.
 *
 * d_Kbb: B x B; d_Keb: Ne x B row-major (a target's kernel row against the background is contiguous); d_Kee: ee_len doubles, model m's
 * csn_m x csn_m block row-major from d_Kee[d_ee_off[m]]; d_en_off: M + 1 ascending int32 row offsets; d_ee_off: M int64 offsets;
 * d_C: M doubles; max_csn: the largest csn_m, ldc = B + max_csn.
 * d_coef: M x ldc, coef[m][t] = a_t y_t for t < n_m (entries past n_m are not written); d_rho, d_gap: M doubles; d_iters (updates
 * made), d_status: M int32.  The gap is that of the returned a.
 * One workgroup per model; no atomics and nothing passes between workgroups; every loop is bounded by max_iter.  Reductions are
 * wavefront shuffles followed by LDS in a fixed order, so a result is the same bits from run to run, and model m's result depends on
 * its own rows of K_eb and K_ee, on K_bb, C_m, eps and max_iter alone -- not on M, the other models or its place in the batch.
 * The kernel reads offsets from the device, so it checks them itself (SC_SVM_BAD_OFFSETS: csn_m outside [1, max_csn], rows outside
 * [0, Ne], a block outside [0, ee_len]) and touches nothing of such a model but its status.
 * Arguments are checked (SK_EARG) before anything is enqueued: a null pointer; B < 1, Ne < 1, M < 1, max_csn < 1, ee_len < 1;
 * B + max_csn > SC_SVM_MAX_N (a problem is never split); eps <= 0 or not a number; max_iter < 1. */
int sc_svm_train(const double* d_Kbb, int32_t B, const double* d_Keb, int32_t Ne, const double* d_Kee, int64_t ee_len,
                 const int32_t* d_en_off, const int64_t* d_ee_off, int32_t M, int32_t max_csn, const double* d_C, double eps,
                 int32_t max_iter, double* d_coef, double* d_rho, int32_t* d_iters, double* d_gap, int32_t* d_status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SIDEKIT_AMD_SVM_H */
