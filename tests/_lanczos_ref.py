"""NumPy restatement of the iteration of vch2d_hess_lanczos: Lanczos on P A P with classical Gram-Schmidt
applied twice, and the device's stop rules.  Pinned by test_lanczos_ref_cpu.py; test_gpu_krylov_2d.py compares the engine's
first steps with it.

    q_0 = P q0 / ||P q0||
    step j: w = P A q_j; twice: c_i = q_i . w for every i of the window (all from the same w), w -= sum_i c_i q_i;
            alpha_j = the two rounds' coefficients on q_j added, beta_j = ||w||
    the window is q_0 .. q_j with reorth, q_{j-1}, q_j without
    stop after min(k, n_free) steps, when beta_j <= 1e-14 max_i |alpha_i|, or when beta_j is not finite
    q_{j+1} = w / beta_j exists unless the step stopped on beta_j or j + 1 == n_free"""
import numpy as np


def lanczos(apply, mask, q0, k, reorth=True):
    """apply: v -> A v on flat vectors; mask: flat booleans; q0: flat start vector.
    Returns dict(alpha, beta: [k] with NaN beyond steps; steps; n_free; Q: the basis vectors that exist, as rows)."""
    mask = np.asarray(mask, dtype=bool).ravel()
    n_free = int(mask.sum())
    if n_free == 0:
        raise ValueError("the free set is empty")
    q = np.where(mask, np.asarray(q0, dtype=np.float64).ravel(), 0.0)
    nrm = float(np.linalg.norm(q))
    if not nrm > 0.0 or not np.isfinite(nrm):
        raise ValueError("the start vector vanishes on the free set")
    Q = [q / nrm]
    alpha, beta = np.full(k, np.nan), np.full(k, np.nan)
    lim, amax, steps = min(int(k), n_free), 0.0, 0
    for j in range(lim):
        w = np.where(mask, apply(Q[j]), 0.0)
        win = Q if reorth else Q[max(j - 1, 0):]
        a = 0.0
        for _ in range(2):
            c = [float(np.dot(v, w)) for v in win]
            for ci, v in zip(c, win):
                w = w - ci * v
            a += c[-1]
        b = float(np.linalg.norm(w))
        alpha[j], beta[j] = a, b
        amax = max(amax, abs(a))
        steps = j + 1
        broke = (not np.isfinite(b)) or b <= 1e-14 * amax
        if not broke and j + 1 < n_free:
            Q.append(w / b)
        if broke or j + 1 >= lim:
            break
    return dict(alpha=alpha, beta=beta, steps=steps, n_free=n_free, Q=np.array(Q))


def ritz(alpha, beta, steps):
    """Ritz values (ascending), the eigenvectors of T and the residual estimates |beta_m s_m| of the first `steps` entries."""
    m = int(steps)
    T = np.diag(alpha[:m]) + np.diag(beta[:m - 1], 1) + np.diag(beta[:m - 1], -1)
    theta, S = np.linalg.eigh(T)
    return theta, S, np.abs(beta[m - 1] * S[m - 1])
