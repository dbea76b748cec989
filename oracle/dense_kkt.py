"""Independent pin for the oracle (test infrastructure, NOT the product).

Assembles the global dense KKT system of an LQ problem exactly as the
reference's test helper does (tests/gar/test_util.hpp:92-165: unknown order
[lbd0, (x_t, u_t, v_t, lbd_{t+1})...], coupling block -I, rhs
[g0; (q, r, d); f; ...], solution = -K^{-1} rhs) and solves it with LAPACK
(numpy.linalg.solve).  Shares no code with gar_oracle.c, so agreement between
the two validates the restated Riccati recursion itself.
"""
from __future__ import annotations

import numpy as np


def lqr_dense_matrix(problem, mueq: float):
    """tests/gar/test_util.hpp:92-165 (``problem``: aligator_amd.lqr.LqrProblem)."""
    knots = problem.stages
    N = problem.horizon
    nc0 = problem.nc0
    nrows = nc0
    for t, k in enumerate(knots):
        nrows += k.nx + k.nu + k.nc
        if t != N:
            nrows += k.nx2          # (lbd_{t+1} has nx2 rows: not nx where the state dimension varies)
    mat = np.zeros((nrows, nrows))
    rhs = np.zeros(nrows)
    nx0 = knots[0].nx
    mat[nc0:nc0 + nx0, :nc0] = problem.G0.T
    mat[:nc0, nc0:nc0 + nx0] = problem.G0
    rhs[:nc0] = problem.g0
    idx = nc0
    for t, m in enumerate(knots):
        n = m.nx + m.nu + m.nc
        blk = mat[idx:idx + n, idx:idx + n]
        blk[:m.nx, :m.nx] = m.Q
        blk[m.nx:m.nx + m.nu, :m.nx] = m.S.T
        blk[:m.nx, m.nx:m.nx + m.nu] = m.S
        blk[m.nx:m.nx + m.nu, m.nx:m.nx + m.nu] = m.R
        blk[m.nx + m.nu:, :m.nx] = m.C
        blk[:m.nx, m.nx + m.nu:] = m.C.T
        blk[m.nx + m.nu:, m.nx:m.nx + m.nu] = m.D
        blk[m.nx:m.nx + m.nu, m.nx + m.nu:] = m.D.T
        blk[m.nx + m.nu:, m.nx + m.nu:] = -mueq * np.eye(m.nc)
        rhs[idx:idx + m.nx] = m.q
        rhs[idx + m.nx:idx + m.nx + m.nu] = m.r
        rhs[idx + m.nx + m.nu:idx + n] = m.d
        if t != N:
            r0 = idx + n
            mat[r0:r0 + m.nx2, idx:idx + m.nx] = m.A
            mat[r0:r0 + m.nx2, idx + m.nx:idx + m.nx + m.nu] = m.B
            mat[r0:r0 + m.nx2, r0 + m.nx2:r0 + 2 * m.nx2] = -np.eye(m.nx2)
            mat[idx:idx + m.nx, r0:r0 + m.nx2] = m.A.T
            mat[idx + m.nx:idx + m.nx + m.nu, r0:r0 + m.nx2] = m.B.T
            mat[r0 + m.nx2:r0 + 2 * m.nx2, r0:r0 + m.nx2] = -np.eye(m.nx2)
            rhs[r0:r0 + m.nx2] = m.f
            idx += n + m.nx2
    return mat, rhs


def dense_solution_to_traj(problem, sol):
    """gar/utils.hpp:79-112 (lqrDenseSolutionToTraj)."""
    N = problem.horizon
    nc0 = problem.nc0
    xs, us, vs, lbdas = [], [], [], [sol[:nc0].copy()]
    idx = nc0
    for t, k in enumerate(problem.stages):
        n = k.nx + k.nu + k.nc
        seg = sol[idx:idx + n]
        xs.append(seg[:k.nx].copy())
        us.append(seg[k.nx:k.nx + k.nu].copy())
        vs.append(seg[k.nx + k.nu:].copy())
        idx += n
        if t < N:
            lbdas.append(sol[idx:idx + k.nx2].copy())
            idx += k.nx2
    return xs, us, vs, lbdas


def dense_solve(problem, mueq: float):
    mat, rhs = lqr_dense_matrix(problem, mueq)
    sol = -np.linalg.solve(mat, rhs)
    return dense_solution_to_traj(problem, sol)
