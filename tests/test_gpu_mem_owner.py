"""Who owns the engines' device and pinned memory (csrc/vch_mem.h), seen from outside through the two diagnostics of
include/vch.h: vch_mem_live() counts the blocks that pools of this process own, vch_mem_refuse_after(k) refuses request k
once without a call to the runtime.  Neither a memory-hungry problem nor a look at the card's free memory is needed (the
card is shared: its free memory is not ours to read).

2D 16 x 16, batch 2, max_steps 4; 1D N = 32, batch 2, max_steps 4.  tests/test_mem_pool_cpu.py checks the pool itself,
sanitised, on the CPU: on a GPU machine run that one first.

1. Balance: create + close, and create + every lazy family + close, bring live back to where it was.
2. Refused create: with n = the allocations of a create, request k refused for every k < n: NULL, a message, live as before.
   Two requests of vch2d_create are the exception the engine has always had: the mapped coherent buffers of the host's looks
   at the device state.  A platform may refuse them, and then the context is created without them (looks
   by copy command).  For exactly those two k the create succeeds with n - 2 blocks, works, and closes to the base; the
   test asserts that there are two such k in 2D, adjacent, and none in 1D.
3. Refused lazy allocation: for each call that allocates lazily, with m = the allocations of its first invocation, request
   k refused for every k < m on a fresh engine: the call raises, the same call repeated succeeds with outputs bit for bit
   those of an engine that never saw a refusal, and close() brings live back.
Every comparison of numbers is bitwise: nothing here is allowed to change a result."""
import numpy as np
import pytest

import vch_amd as V

pytestmark = pytest.mark.gpu

B, M = 2, 4
DT = 1e-2


@pytest.fixture(scope="module")
def lib():
    V.build()
    lib = V.load()
    lib.vch_mem_refuse_after(-1)
    yield lib
    lib.vch_mem_refuse_after(-1)


def eng2d():
    return V.Engine2D(Nx=16, Ny=16, batch=B, max_steps=M)


def eng1d():
    return V.Engine1D(N=32, batch=B, max_steps=M)


@pytest.fixture(scope="module")
def p2():
    """Fixed inputs of the 2D calls (never modified)."""
    x = np.linspace(0.0, 1.0, 17)
    X, Y = np.meshgrid(x, x, indexing="ij")
    rng = np.random.default_rng(7)
    dts = np.full(M, DT)
    t = np.concatenate([[0.0], np.cumsum(dts)])
    phi0 = np.stack([0.1 * np.cos(np.pi * X) * np.cos(2 * np.pi * Y) + 0.05 * b for b in range(B)])
    return dict(x=x, dts=dts, t=t, phi0=phi0, phi_T=0.5 * phi0[::-1].copy(), opt=V.make_opt(),
                U=0.05 * rng.standard_normal((B, M + 1, 17, 17)), H=rng.standard_normal((B, M + 1, 17, 17)),
                R=1e-3 * rng.standard_normal((B, M + 1, 17, 17)), field=rng.standard_normal((B, 17, 17)),
                hist=0.3 * np.tanh(rng.standard_normal((B, M + 1, 17, 17))))


@pytest.fixture(scope="module")
def p1():
    """Fixed inputs of the 1D calls (never modified); histories have M + 2 rows (t = 0 twice)."""
    x = np.linspace(0.0, 1.0, 33)
    rng = np.random.default_rng(11)
    dts = np.full(M, DT)
    t = np.concatenate([[0.0, 0.0], np.cumsum(dts)])
    phi0 = np.stack([0.2 * np.cos(np.pi * x + 0.4 * b) for b in range(B)])
    return dict(x=x, dts=dts, t=t, phi0=phi0, phi_T=0.5 * phi0[::-1].copy(), opt=V.make_opt(),
                U=0.05 * rng.standard_normal((B, M + 2, 33)), H=rng.standard_normal((B, M + 2, 33)),
                R=1e-3 * rng.standard_normal((B, M + 2, 33)), field=rng.standard_normal((B, 33)),
                hist=0.3 * np.tanh(rng.standard_normal((B, M + 2, 33))))


def _flat(res):
    """The arrays of a call's result, in a fixed order, for a bitwise comparison."""
    if isinstance(res, dict):
        return [np.asarray(res[k]) for k in sorted(res) if k not in ("stats", "seconds") and res[k] is not None]
    if isinstance(res, (tuple, list)):
        return [np.asarray(a) for a in res if a is not None and not isinstance(a, dict)]
    return [np.asarray(res)]


def _same(a, b):
    a, b = _flat(a), _flat(b)
    return len(a) == len(b) and all(np.array_equal(u, v, equal_nan=True) for u, v in zip(a, b))


# ---------------------------------------------------------------------------------------------------- 1. balance
def _touch_2d(e, p):
    phi, _ = e.forward(p["phi0"], p["dts"], u=p["U"], store=True)
    e.backward(None, p["t"], 5.0, 10.0, phi_Q=p["hist"], phi_T=p["phi_T"])
    e.second_order(p["H"], p["dts"], p["t"], p["opt"], order=2)      # about the march's own history: before cost() replaces it
    e.hessvec(p["H"], p["dts"], p["t"], p["opt"], order=2)
    e.cost(phi, p["U"], p["hist"], p["phi_T"], p["t"], p["opt"])
    e.free_energy(phi, w_hist=p["hist"])
    e.grad_prox(p["U"], p["R"], 0.5, p["opt"])
    e.prof_begin(64)
    e.apply_laplacian(p["field"])
    e.prof_end()
    e.pgd_init(p["phi0"], p["phi_T"], p["t"], p["opt"], ramp=True)
    e.pgd_iterate(1)
    e.pgd_kkt()


def _touch_1d(e, p):
    phi, _ = e.forward(p["phi0"], p["dts"], u=p["U"], store=True)
    e.backward(None, p["t"], 5.0, 10.0, phi_Q=p["hist"], phi_T=p["phi_T"])
    e.cost(phi, p["U"], p["hist"], p["phi_T"], p["x"], p["t"], p["opt"])
    e.free_energy(phi, w_hist=p["hist"])
    e.grad_prox(p["U"], p["R"], 0.5, p["opt"])
    e.second_order(p["H"], p["t"], p["opt"], u=p["U"], phi_Q=p["hist"], phi_T=p["phi_T"], dt=p["dts"], order=2)
    e.hessvec(p["H"], p["t"], p["opt"], u=p["U"], phi_Q=p["hist"], phi_T=p["phi_T"], dt=p["dts"], order=2)
    e.pgd_init(p["phi0"], p["phi_T"], p["t"], p["dts"], p["opt"])
    e.pgd_iterate(1)
    e.pgd_kkt()


@pytest.mark.parametrize("dim", ["2d", "1d"])
def test_balance(lib, p2, p1, dim):
    make, touch, p = (eng2d, _touch_2d, p2) if dim == "2d" else (eng1d, _touch_1d, p1)
    base = lib.vch_mem_live()
    e = make()
    n = lib.vch_mem_live() - base
    e.close()
    print(dim, "create:", n, "blocks")
    assert n > 10 and lib.vch_mem_live() == base
    e = make()
    touch(e, p)
    full = lib.vch_mem_live() - base
    e.close()
    print(dim, "every lazy family:", full, "blocks")
    assert full > n and lib.vch_mem_live() == base


# ---------------------------------------------------------------------------------------------------- 2. refused create
@pytest.mark.parametrize("dim", ["2d", "1d"])
def test_refused_create(lib, p2, p1, dim):
    make, p = (eng2d, p2) if dim == "2d" else (eng1d, p1)
    base = lib.vch_mem_live()
    e = make()
    n = lib.vch_mem_live() - base
    before = e.apply_laplacian(p["field"]).copy()
    e.close()
    fallback = []
    for k in range(n):
        lib.vch_mem_refuse_after(k)
        try:
            e = make()
        except ValueError as err:
            assert "create failed: " in str(err) and len(str(err)) > len("vch2d_create failed: "), (k, str(err))
            assert lib.vch_last_error() != b""
            assert lib.vch_mem_live() == base, (k, lib.vch_mem_live() - base)
            continue
        finally:
            lib.vch_mem_refuse_after(-1)
        # the look buffers: created without them, and sound
        fallback.append(k)
        assert lib.vch_mem_live() - base == n - 2, (k, lib.vch_mem_live() - base)
        assert np.array_equal(e.apply_laplacian(p["field"]), before)
        e.close()
        assert lib.vch_mem_live() == base
    print(dim, "n =", n, "requests whose refusal the create survives:", fallback)
    assert (len(fallback), fallback[1:]) == ((2, [fallback[0] + 1]) if dim == "2d" else (0, []))
    e = make()
    assert lib.vch_mem_live() - base == n
    assert np.array_equal(e.apply_laplacian(p["field"]), before)
    e.close()
    assert lib.vch_mem_live() == base


# ---------------------------------------------------------------------------------------------------- 3. refused lazy allocation
def _after_forward_2d(e, p):
    e.forward(p["phi0"], p["dts"], u=p["U"], store=False)


def _after_forward_1d(e, p):
    e.forward(p["phi0"], p["dts"], u=p["U"], store=False)


def _pgd_2d(e, p):
    J0 = e.pgd_init(p["phi0"], p["phi_T"], p["t"], p["opt"], ramp=True)
    return [J0, e.pgd_get("phi"), e.pgd_get("phi_Q"), e.pgd_iterate(1), e.pgd_get("u")]


def _pgd_1d(e, p):
    J0 = e.pgd_init(p["phi0"], p["phi_T"], p["t"], p["dts"], p["opt"])
    return [J0, e.pgd_get("phi"), e.pgd_get("phi_Q"), e.pgd_iterate(1), e.pgd_get("u")]


def _flat_pgd(res):
    return [a for part in res for a in _flat(part)]


# name -> (engine, inputs, setup run before the refusal is armed or None, the call); a call returns what is compared
LAZY = {
    "2d_cost": ("2d", None, lambda e, p: e.cost(p["hist"], p["U"], p["hist"][::-1], p["phi_T"], p["t"], p["opt"])),
    "2d_free_energy": ("2d", None, lambda e, p: e.free_energy(p["hist"], w_hist=p["U"])),
    "2d_second_order": ("2d", _after_forward_2d,
                        lambda e, p: e.second_order(p["H"], p["dts"], p["t"], p["opt"], phi_Q=p["hist"], phi_T=p["phi_T"],
                                                    order=2, histories=True)),
    "2d_hessvec": ("2d", _after_forward_2d,
                   lambda e, p: e.hessvec(p["H"], p["dts"], p["t"], p["opt"], phi_Q=p["hist"], phi_T=p["phi_T"], order=2)),
    "2d_pgd_init": ("2d", None, lambda e, p: _flat_pgd(_pgd_2d(e, p))),
    "1d_second_order": ("1d", _after_forward_1d,
                        lambda e, p: e.second_order(p["H"], p["t"], p["opt"], u=p["U"], phi_Q=p["hist"], phi_T=p["phi_T"],
                                                    dt=p["dts"], order=2, histories=True)),
    "1d_hessvec": ("1d", _after_forward_1d,
                   lambda e, p: e.hessvec(p["H"], p["t"], p["opt"], u=p["U"], phi_Q=p["hist"], phi_T=p["phi_T"],
                                          dt=p["dts"], order=2)),
    "1d_pgd_init": ("1d", None, lambda e, p: _flat_pgd(_pgd_1d(e, p))),
}


@pytest.mark.parametrize("name", sorted(LAZY))
def test_refused_lazy_allocation(lib, p2, p1, name):
    dim, setup, call = LAZY[name]
    make, p = (eng2d, p2) if dim == "2d" else (eng1d, p1)
    base = lib.vch_mem_live()
    # a throw-away engine: the allocations of the call's first invocation, and the outputs of an engine without a refusal
    e = make()
    if setup:
        setup(e, p)
    live0 = lib.vch_mem_live()
    want = call(e, p)
    m = lib.vch_mem_live() - live0
    again = call(e, p)
    assert lib.vch_mem_live() - live0 == m and _same(again, want)      # the second invocation allocates nothing
    e.close()
    assert lib.vch_mem_live() == base
    print(name, "m =", m)
    assert m >= 1
    for k in range(m):
        e = make()
        if setup:
            setup(e, p)
        live0 = lib.vch_mem_live()
        lib.vch_mem_refuse_after(k)
        try:
            with pytest.raises((V.VchError, ValueError)):
                call(e, p)
        finally:
            lib.vch_mem_refuse_after(-1)
        assert lib.vch_last_error() != b""
        assert lib.vch_mem_live() - live0 < m, (k, lib.vch_mem_live() - live0)
        got = call(e, p)
        assert lib.vch_mem_live() - live0 == m, (k, lib.vch_mem_live() - live0)
        assert _same(got, want), (name, k)
        e.close()
        assert lib.vch_mem_live() == base, (k, lib.vch_mem_live() - base)
