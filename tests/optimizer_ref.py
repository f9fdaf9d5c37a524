"""Independent restatements of the cache stage's optimizer step for the tests (tests/test_optimizer.py,
tests/test_gpu_optimizer.py): train_step's gradient sanitizing and clipping (internal/train_utils.py:1274-1298,
3154-3161) and optax.adam + apply_updates, in numpy float32 (the element-wise order of rc_adam_update) and in fp64;
a simulation of create_optimizer's chain / masked folding (train_utils.py:3834-3934)."""
import numpy as np

F32_MAX = np.finfo(np.float32).max
F32_EPS = np.finfo(np.float32).eps


def sanitize(g, max_val, dtype):
    """nan_to_num then clip by value (max_val > 0)."""
    g = np.nan_to_num(np.asarray(g, dtype=dtype), nan=0.0, posinf=F32_MAX, neginf=-F32_MAX)
    if max_val > 0:
        g = np.clip(g, dtype(-max_val), dtype(max_val))
    return g


def norm_mult(gs, max_val, max_norm, dtype=np.float64):
    """min(1, max_norm / (FLT_EPSILON + sqrt(sum g^2))) over all buffers, the norm in fp64; -> (norm, mult)."""
    total = sum(float(np.sum(sanitize(g, max_val, np.float64) ** 2)) for g in gs)
    norm = np.sqrt(total)
    if dtype is np.float32:
        n32 = np.float32(norm)
        return n32, np.minimum(np.float32(1), np.float32(max_norm) / (np.float32(F32_EPS) + n32))
    return norm, min(1.0, max_norm / (F32_EPS + norm))


def adam_f32(p, g, mu, nu, grp, sc, mult=None):
    """One rc_adam_update on one buffer in numpy float32, operation by operation.  grp: [n] group index per element;
    sc: train.adam_scalars(...) (per-group lists); mult: the norm-clip multiplier (float32) or None.  -> new p, mu, nu."""
    f = np.float32
    col = lambda k: np.asarray(sc[k], dtype=f)[grp]
    g = sanitize(g, sc["grad_max_val"], f)
    if mult is not None:
        g = f(mult) * g
    mu = col("one_minus_b1") * g + col("b1") * mu
    nu = col("one_minus_b2") * (g * g) + col("b2") * nu
    u = (mu / col("bias_correction1")) / (np.sqrt(nu / col("bias_correction2")) + col("eps"))
    return p + u * (-col("lr")), mu, nu


def adam_f64(p, g, mu, nu, grp, count, groups, b1, b2, eps, max_val=0.0, mult=None):
    """The same step in fp64 from the unrounded hyper-parameters: groups = [schedule dict] (OptimizerConfig.groups())
    and the fp64 learning-rate decay."""
    lr = np.array([lr_decay_f64(count, **s) for s in groups])[grp]
    g = sanitize(g, max_val, np.float64)
    if mult is not None:
        g = mult * g
    mu = (1 - b1) * g + b1 * mu
    nu = (1 - b2) * g * g + b2 * nu
    u = (mu / (1 - b1 ** (count + 1))) / (np.sqrt(nu / (1 - b2 ** (count + 1))) + eps)
    return p - lr * u, mu, nu


def lr_decay_f64(step, lr_init, lr_final, max_steps, lr_delay_steps=0, lr_delay_mult=1.0):
    """math.learning_rate_decay in fp64 (closed form)."""
    if lr_delay_steps > 0:
        rate = lr_delay_mult + (1 - lr_delay_mult) * np.sin(0.5 * np.pi * np.clip(step / lr_delay_steps, 0, 1))
    else:
        rate = 1.0
    t = np.clip(step / max_steps, 0, 1)
    return rate * np.exp(t * (np.log(lr_final) - np.log(lr_init)) + np.log(lr_init))


# ---- optax.chain / optax.masked over a flat tree of names ----------------------------------------------------------
# A transform maps {name: list of Adams applied so far} -> the same with its own effect; masked(tx, mask) runs tx on the
# leaves where mask is True and passes the others through unchanged (optax.masked), chain runs transforms in order.

def adam(label):
    return lambda upd: {k: v + [label] for k, v in upd.items()}


def masked(tx, mask):
    def run(upd):
        inner = tx({k: v for k, v in upd.items() if mask[k]})
        return {k: (inner[k] if mask[k] else v) for k, v in upd.items()}
    return run


def chain(*txs):
    def run(upd):
        for tx in txs:
            upd = tx(upd)
        return upd
    return run


def simulate_groups(names, prefixes):
    """create_optimizer's fold: tx = adam(main); per prefix: chain(masked(tx, prefix not in path),
    masked(adam(prefix), prefix in path)), paths split on "/" below "params".  -> {name: [labels of the Adams]}."""
    parts = {n: n.split("/")[1:] if n.startswith("params/") else n.split("/") for n in names}
    tx = adam("main")
    for p in prefixes:
        tx = chain(masked(tx, {n: p not in parts[n] for n in names}), masked(adam(p), {n: p in parts[n] for n in names}))
    return tx({n: [] for n in names})
