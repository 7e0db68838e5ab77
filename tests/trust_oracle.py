"""Float64 NumPy oracle of the input-trust score (include/psm.h, psm_bind_trust) and the a-priori bounds its tests hold the device to.

Definition, per block row: x the block's S*S*c_in image values in the column order of comp_in ([r][c][ch]), mu and C the mean and
the basis, z the coefficients the score is evaluated at, G = C C^T:

    n   = sum_k (x_k - mu_k)^2
    spe = n - 2 sum_p z_p^2 + z^T G z    ( = |x - mu - C^T z|^2 at z = C (x - mu), for any C )

``score_identity`` evaluates the definition, as the device does, at whatever z it is given; ``score`` the residual norm directly (no
cancellation).  The two agree at z = C (x - mu); at z + delta the definition moves by 2 delta^T (G - 2 I) z + delta^T (G - 2 I) delta,
the residual norm by -2 delta^T (I - G) z + delta^T G delta.

Bounds.  u64 = 2^-53, u32 = 2^-24.  A float64 sum of m terms, in any order, is within m * u64 * sum|terms| of the exact one (to first
order; the factor 2 below covers both sides of a comparison and the rounding of each term).
* ``sum_bound``: what two float64 evaluations of the identity on the SAME x, mu, C, z may differ by.  n: K squares, each with two
  roundings.  sum z^2: P terms.  z^T G z: P^2 products of three factors on top of G's own K-term sums, |G_pq| <= |C_p| |C_q|, so
  sum |z_p G_pq z_q| <= (sum_p |z_p| |C_p|)^2 =: A.   bound = 2 u64 [ (K + 2) n + 2 (P + 2) |z|^2 + (P^2 + P + K + 4) A ].
* ``storage_bound``: what rounding mu and C to float32 moves a squared residual norm rho^2 by: the residual vector moves by at most
  e = u32 (|mu| + |C|_F |z|), so rho^2 by at most 2 rho e + e^2.
* ``coefficient_bound``: what evaluating the residual norm at z~ = z + delta instead of z = C (x - mu) moves it by: at most
  2 |delta| |(I - G) z| + |G|_2 |delta|^2.
"""
import numpy as np

U64, U32 = 2.0 ** -53, 2.0 ** -24


def blocks_of(image, origins, S, c_in):
    """[B, S*S*c_in] float64 rows of one case's image [Ny, Nx, >= c_in], the reference's reshape."""
    img = np.asarray(image)
    return np.stack([np.asarray(img[y0:y0 + S, x0:x0 + S, :c_in], np.float64).reshape(-1) for y0, x0 in origins])


def encode(x, mu, C):
    """z = C (x - mu), all float64: [B, P]."""
    return (np.asarray(x, np.float64) - np.asarray(mu, np.float64)) @ np.asarray(C, np.float64).T


def score(x, mu, C, z):
    """(n, |x - mu - C^T z|^2) [B], both as direct sums of squares."""
    r = np.asarray(x, np.float64) - np.asarray(mu, np.float64)
    rho = r - np.asarray(z, np.float64) @ np.asarray(C, np.float64)
    return np.einsum("bk,bk->b", r, r), np.einsum("bk,bk->b", rho, rho)


def score_identity(x, mu, C, z):
    """(n, spe) [B] of the definition: spe = n - 2 |z|^2 + z^T G z; n == 0 gives spe = 0."""
    C = np.asarray(C, np.float64)
    z = np.asarray(z, np.float64)
    r = np.asarray(x, np.float64) - np.asarray(mu, np.float64)
    n = np.einsum("bk,bk->b", r, r)
    spe = n - 2.0 * np.einsum("bp,bp->b", z, z) + np.einsum("bp,pq,bq->b", z, C @ C.T, z)
    return n, np.where(n == 0.0, 0.0, spe)


def unscale(xin, model):
    """The device's coefficients: PSM_STAGE_X_INPUT rows [M, p_in] float32 with the input scaler undone in float64, through the
    float32 factors the handle stores (x_in = z * ia + ib, psm_set_scaler)."""
    P = model.p_in
    a, b = np.broadcast_to(np.asarray(model.in_a, np.float64), (P,)), np.broadcast_to(np.asarray(model.in_b, np.float64), (P,))
    if model.scaler_kind == "max_abs":
        ia, ib = 1.0 / a, np.zeros(P)
    elif model.scaler_kind == "std":
        ia, ib = 1.0 / b, -a / b
    else:
        ia, ib = 1.0 / (b - a), -a / (b - a)
    ia, ib = ia.astype(np.float32).astype(np.float64), ib.astype(np.float32).astype(np.float64)
    return (np.asarray(xin, np.float64) - ib) / ia


def sum_bound(n, z, C, K):
    z = np.abs(np.asarray(z, np.float64))
    P = z.shape[-1]
    rows = np.linalg.norm(np.asarray(C, np.float64), axis=1)
    A = (z @ rows) ** 2
    return 2.0 * U64 * ((K + 2) * np.asarray(n, np.float64) + 2.0 * (P + 2) * np.einsum("bp,bp->b", z, z) + (P * P + P + K + 4) * A)


def storage_bound(rho2, z, mu, C):
    e = U32 * (np.linalg.norm(mu) + np.linalg.norm(C) * np.linalg.norm(np.asarray(z, np.float64), axis=-1))
    return 2.0 * np.sqrt(np.maximum(np.asarray(rho2, np.float64), 0.0)) * e + e * e


def coefficient_bound(delta, z, C):
    C = np.asarray(C, np.float64)
    G = C @ C.T
    d = np.linalg.norm(np.asarray(delta, np.float64), axis=-1)
    slack = np.linalg.norm(np.asarray(z, np.float64) @ (np.eye(G.shape[0]) - G), axis=-1)
    return 2.0 * d * slack + np.linalg.norm(G, 2) * d * d
