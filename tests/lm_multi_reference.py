"""What the multi-start Levenberg-Marquardt kernels are held against (``ehr_lm_update_multi``, easyhec_amd/lm_multi.py):

* ``update_multi``: one ``ehr_lm_update_multi`` call IS a loop of ``lm_reference.update`` over the hypotheses, each on its own
  views, pose, and state -- there is no arithmetic across hypotheses to restate.
* ``system`` / ``scripted_calls``: the inputs of the update-kernel test.  The systems are generated as
  tests/test_gpu_lm.py's ``system(N, B, seed)`` generates them (restated here so that the CPU tests can use them: that file
  needs a GPU to import); the losses are SCRIPTED per hypothesis so that the inputs alone decide which calls are accepted,
  rejected, reported, and which call stops a hypothesis.  tests/test_lm_multi_reference.py pins the script on the CPU."""
import numpy as np

import lm_reference as LR

FTOL = 1e-12   # as tests/test_gpu_lm.py: the synthetic systems' predicted reductions are small next to their losses
# Where the systems' seeds start.  Chosen on the CPU with ``lm_reference.update`` among 0, 1000, ..., 119000: the first for which
# every call of SCRIPT does what it says at N = 1 and 6, (P, Bv) = (1, 1) and (3, 2), with the smallest predicted reduction of
# a call that must NOT stop 6.4 x ftol F (N = 1 systems are nearly solved by their first step; most seeds stop one early).
SEED0 = 108000


def update_multi(states, info, grad, count, loss, dof, Bv, N, ftol=1e-6, lambda_max=1e6, finalize=False):
    """states: P ``lm_reference.new_state()``; info [P*Bv,N,N], grad [P*Bv,N], count [P*Bv], loss [P*Bv]; dof [P,6] float32,
    modified in place (the first N coordinates of each row are the parameters).  Returns dof."""
    for p, st in enumerate(states):
        v = slice(p * Bv, (p + 1) * Bv)
        dof[p, :N] = LR.update(st, info[v], grad[v], count[v], loss[v], dof[p, :N].copy(), ftol, lambda_max, finalize)
    return dof


def system(N, B, seed):
    """tests/test_gpu_lm.py's ``system``: info [B,N,N] SPD, scaled condition number <= 1e6, parameters of different units;
    grad = 2 H x for a small x."""
    rng = np.random.default_rng(77 * N + seed)
    scale = 10.0 ** rng.uniform(-2, 2, N)
    info = np.zeros((B, N, N))
    for b in range(B):
        Q, _ = np.linalg.qr(rng.normal(size=(N, N)))
        M = (Q * 10.0 ** rng.uniform(-5, 0, N)) @ Q.T
        info[b] = 0.5 * (M + M.T) * scale[:, None] * scale[None, :]
    x = rng.normal(size=N) * 1e-3 / scale
    grad = np.stack([2.0 * info[b] @ x for b in range(B)])
    return info, grad, rng.integers(10, 500, B), rng.uniform(10, 100, B).astype(np.float32)


# Per hypothesis and call: the loss as a factor of the hypothesis's first loss, and what that makes of the call --
# "a" accepted (the first call, or a loss strictly below every earlier accepted one), "r" rejected, "s" accepted with a zero
# gradient (predicted reduction 0 <= ftol F: the ftol rule stops the hypothesis), "n" a NaN in the call's grad (reported),
# "-" the hypothesis is done and the call only restores its pose.
SCRIPT = [
    [(1.0, "a"), (0.9, "a"), (1.5, "r"), (2.0, "r"), (0.8, "s"), (0.7, "-"), (0.6, "-")],
    [(1.0, "a"), (1.2, "r"), (0.9, "a"), (0.85, "a"), (1.5, "r"), (0.8, "n"), (0.7, "a")],
    [(1.0, "a"), (0.95, "a"), (0.9, "a"), (1.1, "r"), (0.85, "a"), (0.8, "a"), (0.75, "a")],
]
CALLS = len(SCRIPT[0])


def start_dof(P, seed=0):
    """[P,6] float32 poses the update test starts from."""
    return np.random.default_rng(4242 + seed).uniform(-1, 1, (P, 6)).astype(np.float32)


def scripted_calls(N, P, Bv):
    """A list of CALLS tuples ``(info [P*Bv,N,N], grad [P*Bv,N], count [P*Bv], loss [P*Bv] float32)``: hypothesis p's views of
    call c are ``system(N, Bv, SEED0 + 100 * p + c)`` -- a different system per hypothesis, fresh inputs per call -- with the loss
    scaled, the gradient zeroed or a NaN planted as ``SCRIPT[p][c]`` says."""
    assert P <= len(SCRIPT)
    base = [system(N, Bv, SEED0 + 100 * p)[3] for p in range(P)]
    calls = []
    for c in range(CALLS):
        parts = []
        for p in range(P):
            info, grad, count, _ = system(N, Bv, SEED0 + 100 * p + c)
            factor, what = SCRIPT[p][c]
            if what == "s":
                grad = np.zeros_like(grad)
            if what == "n":
                grad = grad.copy()
                grad[Bv - 1, N - 1] = np.nan
            parts.append((info, grad, count, (base[p] * np.float32(factor)).astype(np.float32)))
        calls.append(tuple(np.concatenate([x[i] for x in parts]) for i in range(4)))
    return calls


def expected_flags(p, c):
    """(last, done) the state of hypothesis p shows after call c, from SCRIPT alone."""
    what = SCRIPT[p][c][1]
    done = any(SCRIPT[p][k][1] == "s" for k in range(c + 1))
    if what == "-":
        k = max(i for i in range(c) if SCRIPT[p][i][1] != "-")
        what = SCRIPT[p][k][1]
    return {"a": 1, "s": 1, "r": 0, "n": -1}[what], int(done)
