"""A batch of LQ problems as a differentiable PyTorch layer: LqSolve / LqLayer on a BatchedRiccatiSolver.

forward:  packed (batch x problem_doubles, the caller's packed layout -- BatchedRiccatiSolver.pack -- on the solver's
          device) -> upload_packed_user_device, backward_async(mueq), forward_async, solution_vectors_device -> the solutions
          (batch x affine_doubles: x_t | u_t | lbd_{t+1} per stage, then lbd0)
backward: the incoming cotangent -> adjoint_async (csrc/gar_adjoint.hpp) -> the gradient of `packed`, same shape

Everything is enqueued on torch's current stream; nothing here waits for the device.  A problem whose backward sweep
fails (status word != 0) contributes a zero gradient; its solution is whatever the roll-out left.  `solver.status()`
after a forward tells which -- the layer does not read it by itself (that would be a host synchronisation).
One solver, one batch: the layer does not resize it.  The gradient with respect to mueq is not formed.
backward differentiates what the solver HOLDS: it must run before the next forward on the same solver (a later forward makes
the earlier graph's backward raise); whoever drives the solver directly between the two (upload, backward, refine)
is on their own.  The layer also owns the solver's stream: after a direct solver.set_stream, call forget_stream(solver).
On the emulator build of the library device pointers are host pointers: the same layer runs on CPU tensors there.
lq_affine_solve_multi(solver, rhs) solves the batch the solver holds for many sets of affine terms at once, on the same
stream discipline (no autograd: it is the adjoint solve itself, for several cotangents)."""
import torch

from .gar import BatchedRiccatiSolver


def _set_stream(solver: BatchedRiccatiSolver, handle: int):
    if getattr(solver, "_layer_stream_handle", None) != handle:      # (set_stream drains the stream it leaves)
        solver.set_stream(handle)
        solver._layer_stream_handle = handle


def forget_stream(solver: BatchedRiccatiSolver):
    """after the caller moved the solver to another stream itself: the layer sets its own again on the next call"""
    solver._layer_stream_handle = None


def _begin(solver: BatchedRiccatiSolver, like: torch.Tensor):
    """the solver onto torch's current stream.  The legacy default stream has the null handle, which the library reads as
    "your own stream": then the work goes to a side stream of the layer's, ordered behind and ahead of the current one"""
    if not like.is_cuda:
        return None
    cur = torch.cuda.current_stream(like.device)
    if cur.cuda_stream != 0:
        _set_stream(solver, cur.cuda_stream)
        return None
    side = getattr(solver, "_layer_stream", None)
    if side is None:
        side = solver._layer_stream = torch.cuda.Stream(like.device)
    side.wait_stream(cur)
    _set_stream(solver, side.cuda_stream)
    return cur, side


def _end(token, tensors):
    if token is not None:
        cur, side = token
        cur.wait_stream(side)
        for t in tensors:
            t.record_stream(side)


class LqSolve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, packed: torch.Tensor, solver: BatchedRiccatiSolver, mueq: float):
        if packed.dtype != torch.float64 or tuple(packed.shape) != (solver.batch, solver.problem_doubles):
            raise ValueError(f"packed must be float64 of shape ({solver.batch}, {solver.problem_doubles}), "
                             f"got {packed.dtype} {tuple(packed.shape)}")
        src = packed.detach().contiguous()
        out = torch.empty((solver.batch, solver.affine_doubles), dtype=torch.float64, device=packed.device)
        token = _begin(solver, packed)
        solver.upload_packed_user_device(src.data_ptr())
        solver.backward_async(mueq)
        solver.forward_async()
        solver.solution_vectors_device(out.data_ptr())
        _end(token, (src, out))
        solver._layer_generation = getattr(solver, "_layer_generation", 0) + 1
        ctx.solver, ctx.generation = solver, solver._layer_generation
        ctx.shape = tuple(packed.shape)
        return out

    @staticmethod
    def backward(ctx, cot: torch.Tensor):
        solver = ctx.solver
        if solver._layer_generation != ctx.generation:
            raise RuntimeError("LqSolve.backward: another forward ran on this solver since this graph's forward -- the "
                               "solver holds that batch now (one solver, one batch: differentiate before the next forward)")
        cot = cot.contiguous()
        grad = torch.empty(ctx.shape, dtype=torch.float64, device=cot.device)
        token = _begin(solver, cot)
        solver.adjoint_async(cot.data_ptr(), 0, grad.data_ptr())
        _end(token, (cot, grad))
        return grad, None, None


def lq_affine_solve_multi(solver: BatchedRiccatiSolver, rhs: torch.Tensor) -> torch.Tensor:
    """rhs (batch, nrhs, affine_doubles), float64 on the solver's device: for every problem, nrhs sets of affine terms (q_t
    | r_t | f_t per stage, then g0).  -> the LQ solutions for the matrices the solver holds and those terms, same shape
    (affine_solve_multi_async, csrc/gar_affine_multi.hpp).  Enqueued on torch's current stream, not waited for; not
    differentiable (no graph is recorded).  The solver needs a backward whose matrices are still current."""
    if rhs.dtype != torch.float64 or rhs.dim() != 3 or rhs.shape[0] != solver.batch or rhs.shape[2] != solver.affine_doubles:
        raise ValueError(f"rhs must be float64 of shape ({solver.batch}, nrhs, {solver.affine_doubles}), "
                         f"got {rhs.dtype} {tuple(rhs.shape)}")
    src = rhs.detach().contiguous()
    out = torch.empty_like(src)
    token = _begin(solver, src)
    solver.affine_solve_multi_async(src.data_ptr(), int(src.shape[1]), out.data_ptr())
    _end(token, (src, out))
    return out


class LqLayer(torch.nn.Module):
    """layer(packed) -> solutions, differentiable with respect to `packed`; `solver` holds the batch between calls"""

    def __init__(self, solver: BatchedRiccatiSolver, mueq: float = 1e-10):
        super().__init__()
        self.solver = solver
        self.mueq = float(mueq)

    def forward(self, packed: torch.Tensor) -> torch.Tensor:
        return LqSolve.apply(packed, self.solver, self.mueq)
