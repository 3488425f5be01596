"""float64 restatement of the C51 head ALONE (model.py:74-79, agent.py:66-96) — TEST INFRASTRUCTURE.

Input: the [3B, NZ] logits exactly as the implementation under test produced them (rb_learner_debug_read selector 4: rows
[0, B) online(states), [B, 2B) online(next_states), [2B, 3B) target(next_states); a row is Z value logits followed by A x Z
advantage logits), the batch scalars and the config.  Feeding the head's own input isolates it from the convs and FC layers
in front of it: a head bug cannot hide inside upstream summation noise, and upstream noise cannot flip an argmax.

Precision: the bin position b = (clamp(R + nt * gamma^n * z) - Vmin) / dz and with it l, u are DISCRETE decisions; they are
formed in float32, operation for operation as oracle.learner_oracle.project and csrc/head.h form them, so that they do not
move with precision.  Everything else (dueling combine, softmaxes, expected values, the projected mass, loss, d loss / d
logits) is float64."""
import numpy as np

from oracle import learner_oracle as O


def support32(cfg):
    """torch.linspace(Vmin, Vmax, Z) in float32 (agent.py:18): the values the head reads."""
    return O.support(cfg).numpy().astype(np.float32)


def dueling(lg, Z, A):
    """q = v + a - mean_a(a)  (model.py:74-75); lg [n, NZ] -> [n, A, Z], float64."""
    lg = np.asarray(lg, dtype=np.float64)
    v = lg[:, :Z].reshape(-1, 1, Z)
    a = lg[:, Z:].reshape(-1, A, Z)
    return v + a - a.mean(axis=1, keepdims=True)


def log_softmax(q):
    q = q - q.max(axis=-1, keepdims=True)
    return q - np.log(np.exp(q).sum(axis=-1, keepdims=True))


def expected_values(cfg, lg):
    """sum_z z p(z) per action (agent.py:72 / :54); lg [n, NZ] -> [n, A], float64."""
    p = np.exp(log_softmax(dueling(lg, cfg.atoms, cfg.actions)))
    return (p * support32(cfg).astype(np.float64)).sum(axis=2)


def top2_gap(ev):
    """Per row: best minus second-best value (inf with one action)."""
    ev = np.asarray(ev, dtype=np.float64)
    if ev.shape[1] < 2:
        return np.full(ev.shape[0], np.inf)
    s = np.sort(ev, axis=1)
    return s[:, -1] - s[:, -2]


def bins32(cfg, returns, nonterminals):
    """(Tz unclamped f32, b f32, l, u) of agent.py:79-86, the float32 chain of project() / k_head."""
    Z = cfg.atoms
    f = np.float32
    R = np.asarray(returns, dtype=f).reshape(-1, 1)
    nt = np.asarray(nonterminals, dtype=f).reshape(-1, 1)
    gamma_n = f(cfg.discount ** cfg.multi_step)
    delta_z = f((cfg.v_max - cfg.v_min) / (Z - 1))
    raw = (R + (nt * gamma_n) * support32(cfg).reshape(1, Z)).astype(f)               # agent.py:79
    Tz = np.minimum(np.maximum(raw, f(cfg.v_min)), f(cfg.v_max))                      # agent.py:80
    b = ((Tz - f(cfg.v_min)) / delta_z).astype(f)                                     # agent.py:82
    assert raw.dtype == f and Tz.dtype == f and b.dtype == f
    l, u = np.floor(b).astype(np.int64), np.ceil(b).astype(np.int64)                  # agent.py:83
    l = np.where((u > 0) & (l == u), l - 1, l)                                        # agent.py:85
    u = np.where((l < Z - 1) & (l == u), u + 1, u)                                    # agent.py:86
    return raw, b, l, u


def head(cfg, logits, actions, returns, nonterminals, weights):
    """The whole head of one learn call.  Returns float64 arrays (int64 for a_star, l, u):
    log_ps_a [B, Z], ev [B, A], a_star [B], gap [B] (top-2 gap of ev), pns_a [B, Z], m [B, Z], l / u [B, Z], b [B, Z]
    (float32 values), loss [B], dlogits [B, NZ] (of mean(w * loss), dueling adjoint included)."""
    B, Z, A = cfg.batch, cfg.atoms, cfg.actions
    NZ = Z * (A + 1)
    lg = np.asarray(logits, dtype=np.float64)
    assert lg.shape == (3 * B, NZ), lg.shape
    actions = np.asarray(actions, dtype=np.int64).reshape(B)
    w = np.asarray(weights, dtype=np.float64).reshape(B)
    rows = np.arange(B)
    log_ps = log_softmax(dueling(lg[:B], Z, A))                                       # agent.py:66
    log_ps_a = log_ps[rows, actions]                                                  # agent.py:67
    ev = expected_values(cfg, lg[B:2 * B])                                            # agent.py:71-72
    a_star = ev.argmax(axis=1)                                                        # agent.py:73
    pns_a = np.exp(log_softmax(dueling(lg[2 * B:], Z, A)))[rows, a_star]              # agent.py:75-76
    _raw, b32, l, u = bins32(cfg, returns, nonterminals)
    b = b32.astype(np.float64)
    m = np.zeros((B, Z), dtype=np.float64)
    for i in range(B):
        np.add.at(m[i], l[i], pns_a[i] * (u[i] - b[i]))                               # agent.py:91
        np.add.at(m[i], u[i], pns_a[i] * (b[i] - l[i]))                               # agent.py:92
    loss = -(m * log_ps_a).sum(axis=1)                                                # agent.py:94
    # d mean(w * loss) / d q[b, act, z] = (w_b / B) (p[z] sum(m) - m[z]); q = v + a - mean_a(a):
    # dv = g, da[a'] = (delta(a', act) - 1 / A) g                                      agent.py:96
    g = (w / B).reshape(B, 1) * (np.exp(log_ps_a) * m.sum(axis=1, keepdims=True) - m)
    da = np.repeat((-g / A)[:, None, :], A, axis=1)
    da[rows, actions] += g
    dlogits = np.concatenate([g, da.reshape(B, A * Z)], axis=1)
    return dict(log_ps_a=log_ps_a, ev=ev, a_star=a_star, gap=top2_gap(ev), pns_a=pns_a, m=m, l=l, u=u, b=b32, loss=loss,
                dlogits=dlogits)
