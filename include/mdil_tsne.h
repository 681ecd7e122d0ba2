/*
 * libmdil_tsne.so -- C ABI of the latent-space add-on: exact t-SNE (2 components, 1 degree of
 * freedom) on the device, in three steps that mirror sklearn.manifold._t_sne:
 *
 *   mdil_tsne_sqdist      pairwise squared distances        (pairwise_distances(squared=True))
 *   mdil_tsne_affinities  per-row perplexity search + joint (_joint_probabilities)
 *   mdil_tsne_run         `iters` gradient-descent steps    (_gradient_descent on _kl_divergence)
 *
 * A fifth library, beside libmdil_hip.so and the three inference add-ons: nothing of any of them
 * is compiled into it or changed by it ("Latent space").  Same conventions as
 * include/mdil_predict.h:
 *
 *   - plain pointers and sizes only; every pointer is DEVICE memory owned by the caller; the
 *     library allocates nothing, keeps no state but the thread-local error text, and every call is
 *     re-entrant (on different workspaces).
 *   - `stream` is a hipStream_t passed as void*; the work is enqueued there, no implicit sync and
 *     no host synchronisation inside any call.
 *   - return 0 on success, negative on error; mdil_tsne_last_error() gives thread-local text.
 *   - no float atomics: every reduction runs in a fixed order, so equal inputs give equal bits.
 *
 * What is NOT here, against sklearn: the two early-stopping criteria of _gradient_descent
 * (n_iter_without_progress, min_grad_norm) -- a fixed iteration count is what lets
 * mdil_tsne_run enqueue everything without reading anything back; and the 2.22e-16 clamp on Q,
 * which cannot act in fp32 for finite Y: q_ij = n_ij / Z >= 1 / ((1 + d^2) N^2), and d^2 overflows
 * the format long before that reaches 1e-16.  P is fp32 and dense.
 */
#ifndef MDIL_TSNE_H
#define MDIL_TSNE_H

#ifdef __cplusplus
extern "C" {
#endif

#define MDIL_TSNE_OK 0
#define MDIL_TSNE_ERR_INVALID (-1)
#define MDIL_TSNE_ERR_LAUNCH (-2)

#define MDIL_TSNE_MAX_POINTS 32768
#define MDIL_TSNE_MAX_DIM 128
#define MDIL_TSNE_MAX_SEARCH_STEPS 100
#define MDIL_TSNE_ENTROPY_TOL 1e-5

int mdil_tsne_version(void);
const char* mdil_tsne_last_error(void);

/* Bytes of the `workspace` of mdil_tsne_affinities and of the `partials` of mdil_tsne_run for N
 * points (one buffer of this size serves both, one call at a time); 16-byte aligned.  -1 when N is
 * outside [2, MDIL_TSNE_MAX_POINTS]. */
long long mdil_tsne_workspace_bytes(int N);

/* X f32 [N][d] row-major, 2 <= N <= 32768, 1 <= d <= 128  ->  D f32 [N][N],
 *      D[i][j] = sum_k (x_ik - x_jk)^2      k ascending, each term one subtraction and one FMA
 * formed from the differences (never |x|^2 + |y|^2 - 2xy), so D[i][i] == 0 exactly and
 * D[i][j] == D[j][i] bit for bit. */
int mdil_tsne_sqdist(const float* X, int N, int d, float* D, void* stream);

/* D f32 [N][N] (squared distances)  ->  beta_out f64 [N], P f32 [N][N].
 * Per row i, sklearn's _binary_search_perplexity: beta = 1; at most 100 steps of
 *      p_j = exp(-beta D_ij) (j != i), S = sum_j p_j (0 -> 1e-8), H = log S + beta sum_j D_ij p_j / S;
 *      stop when |H - log(perplexity)| <= 1e-5; H too large: beta doubles until bracketed, then
 *      bisects upward; H too small: halves / bisects downward
 * with exp, both sums and H in fp64 (the sums in a fixed order).  beta_out[i] is the beta the row's
 * probabilities were LAST EVALUATED at.  With C[i][j] = p_j / S (fp32, C[i][i] = 0)
 *      P[i][j] = max((C[i][j] + C[j][i]) / max(sum(C + C^T), 2.22e-16), 2.22e-16)  (i != j),  P[i][i] = 0
 * (the sum in fp64, fixed order), bitwise symmetric.  D and P must not overlap; both 16-byte
 * aligned.  perplexity must be >= 1 and < N.  workspace: mdil_tsne_workspace_bytes(N). */
int mdil_tsne_affinities(const float* D, int N, double perplexity, double* beta_out, float* P,
                         void* workspace, void* stream);

/* Enqueues iterations it = 0 .. iters-1 of sklearn's _gradient_descent on the exact
 * _kl_divergence.  P f32 [N][N] MUST be symmetric with a zero diagonal (what mdil_tsne_affinities
 * writes): row i of the sweep is read as column i.  Y, update, gains: f32 [N][2], read and written.
 * Per iteration, with g = first_iter + it, e = (g < exaggeration_iters ? exaggeration : 1),
 * momentum = (g < exaggeration_iters ? 0.5 : 0.8), n_ij = 1 / (1 + |y_i - y_j|^2):
 *      Z = sum_{i != j} n_ij,   grad_i = 4 (e sum_j p_ij n_ij (y_i - y_j) - sum_j n_ij^2 (y_i - y_j) / Z)
 *      inc = update * grad < 0;  gains = max(inc ? gains + 0.2 : gains * 0.8, 0.01)
 *      update = momentum * update - learning_rate * (gains * grad);  Y += update
 * and, as sklearn's TSNE runs the two phases as two _gradient_descent calls, the iteration with
 * g == exaggeration_iters first takes update = 0 and gains = 1 in place of what is stored.
 * When kl_every > 0, every iteration with it % kl_every == kl_every - 1 also writes
 *      kl_log[2 (it / kl_every)]     = KL(e P || Q) at the Y the iteration STARTED from
 *                                    = e (S log e + sum p log p - sum_ij p_ij log n_ij + S log Z), S = sum p
 *      kl_log[2 (it / kl_every) + 1] = |grad|_2 of that iteration
 * (what sklearn reports: during the exaggeration phase the divergence of the exaggerated P).
 * kl_log: f32 [iters / kl_every][2], may be NULL when kl_every <= 0.  sum p log p is formed once per
 * call.  partials: mdil_tsne_workspace_bytes(N), 16-byte aligned like P.  A run split over several
 * calls (first_iter advancing) equals one call bit for bit in Y, update and gains; which iterations are
 * logged follows the call's own `it`, so the calls' kl_logs line up with the single call's only when every
 * split point is a multiple of kl_every.  No early stopping (see above). */
int mdil_tsne_run(const float* P, int N, float* Y, float* update, float* gains, int iters,
                  int first_iter, int exaggeration_iters, float exaggeration, float learning_rate,
                  int kl_every, float* kl_log, void* partials, void* stream);

#ifdef __cplusplus
}
#endif
#endif
