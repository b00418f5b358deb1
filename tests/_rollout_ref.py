"""Plain float64 restatements (numpy / torch on the CPU) of what the persistent shared-std Gaussian rollout, its value
pass and the GAE / discounted-return scan compute (torchrl_amd/csrc/k_rollout.hip: rollout_kernel, value_pass_kernel;
k_gae.hip) -- test infrastructure, imported by tests/test_rollout_kernels_*.py and tests/test_rollout_heads_*.py only.
Written from the formulas of oracle/collector.py, oracle/synth_env.py and oracle/replay.py; log pi, the explore step and the
normaliser are those of tests/_gauss_ref.py.  A case's `head` selects the rollout kernel's other two policy heads: "cat", the
categorical draw of tests/_categorical_ref.py (`cat_terms`), and "sd", the state-dependent-std Gaussian of
tests/_gauss_sd_ref.py (`sd_logp_terms`); everything that does not depend on the head is one code path.

A CASE is a dict of planted inputs (`rollout_case`, `norm_case`, `gae_case`); a RUN is the dict of arrays a launch leaves
behind (the GPU file reads it back from the device, `emulate` produces it on the CPU in float32 or float64); `verify`,
`verify_norm_step` and `scan_ratios` compare a run with the restatement TEACHER-FORCED: every stored (t, n) is restated from
the run's own obs[t, n] and the step's noise, so no error accumulates over the steps.  Each compared quantity has a derived
bound; the functions return the worst err / bound per quantity and assert the exact parts themselves."""
import numpy as np
import torch

import _categorical_ref as CR
import _gauss_ref as G
from oracle import nets, philox, replay
from oracle.synth_env import dynamics_matrices

U = G.U                                                         # 2^-24, the float32 unit round-off
SENT = -777.25                                                  # pre-fill of everything a launch may write
RESET_ATOL = 3e-6                                               # Philox normals, test_kernels_gpu.py::test_synth_reset_vs_oracle_philox
DISCOUNT = 0.99
F32 = lambda x: float(np.float32(x))
ACT_FN = {"tanh": np.tanh, "relu": lambda x: np.maximum(x, 0.0)}


# ------------------------------------------------------------------ networks
def mlp(params, x, act, dtype=np.float64):
    """Two hidden layers and a linear head; params [W1, b1, W2, b2, W3, b3], W (out, in)."""
    p = [np.asarray(q.detach().numpy() if torch.is_tensor(q) else q).astype(dtype) for q in params]
    h = np.asarray(x).astype(dtype)
    for k in range(2):
        h = ACT_FN[act](h @ p[2 * k].T + p[2 * k + 1]).astype(dtype)
    return (h @ p[4].T + p[5]).astype(dtype)


def make_nets(D, A, seed, head="gauss", head_scale=30.0, ls_bias=-1.5, stress=None, tie=None, peak=None):
    """oracle.nets.init_mlp with the policy head's weights times 30 and its biases times 100 (+-0.3): means (logits) of a
    few tenths; the value head's weights times 100: values of a few tenths.
    head "cat": A logits, the weights times `head_scale` (3000: a peaked head, logits of tens).  tie = b: head rows 1 and
    A - 1 are made bit-identical (row 1's weights, row 1's bias + b), so the two logits are the same float in any arithmetic;
    peak = b: row 2's bias + b.
    head "sd": 2A rows [mean | raw log_std], the log_std biases at `ls_bias`.  stress = (kind, ls_scale, ls_bias): the stress
    heads of tests/_gauss_sd_rollout_ref.py::STRESS_CASES -- the log_std rows are the initialiser's times ls_scale and their
    biases ls_bias ("span"); "pinned": also the LAST dim's bias at -25 (always on the lower clamp) and the FIRST at +3."""
    gen = torch.Generator().manual_seed(seed)
    rows = 2 * A if head == "sd" else A
    pf, vf = nets.init_mlp(D, [64, 64], rows, generator=gen), nets.init_mlp(D, [64, 64], 1, generator=gen)
    raw_w = pf[4].clone()
    pf[4], pf[5], vf[4] = pf[4] * 30.0, pf[5] * 100.0, vf[4] * 100.0
    if head == "cat":
        pf[4] = raw_w * float(head_scale)
        if tie is not None:
            pf[4][A - 1] = pf[4][1]
            pf[5][1] = pf[5][1] + float(tie)
            pf[5][A - 1] = pf[5][1]
        if peak is not None:
            pf[5][min(2, A - 1)] += float(peak)
    elif head == "sd":
        pf[5][A:] = float(ls_bias)
        if stress is not None:
            kind, ls_scale, bias = stress
            pf[4][A:] = raw_w[A:] * float(ls_scale)
            pf[5][A:] = float(bias)
            if kind == "pinned":
                pf[5][2 * A - 1], pf[5][A] = -25.0, 3.0
    return pf, vf


def flat(params, logstd=None):
    parts = [p.reshape(-1).float() for p in params] + ([] if logstd is None else [logstd.reshape(-1).float()])
    return torch.cat(parts).contiguous()


# ------------------------------------------------------------------ cases of the rollout tests
INSTANCES = [  # (D, A, act, tanh_action): the compile-time benchmark shape, then the runtime-dims Gaussian instantiations
    (17, 6, "tanh", True), (17, 6, "relu", True),
    (5, 3, "tanh", True), (17, 6, "tanh", False), (18, 1, "relu", True), (32, 8, "tanh", True), (4, 1, "tanh", True)]
ROLL_N, ROLL_T = (1, 15, 16, 17, 40), (1, 5, 12)
KINDS = ("done", "over", "both", "neither", "neither")


def plant_counters(N, T, horizon, max_frames):
    """Envs out of step: env n is of kind KINDS[n % 5] and its event falls in step (7 n + 1) % T of the launch; after
    a reset the counters restart at 0 and T < max_frames < horizon keeps a second event out of the launch."""
    assert T < max_frames < horizon
    t_env, cur_step = np.zeros(N, np.int32), np.zeros(N, np.int32)
    for n in range(N):
        s, kind = (7 * n + 1) % T, KINDS[n % 5]
        if kind in ("done", "both"):
            t_env[n] = horizon - 1 - s
        else:
            t_env[n] = n % 3
        if kind in ("over", "both"):
            cur_step[n] = max_frames - 1 - s
        else:
            cur_step[n] = n % 2
    return t_env, cur_step


def rollout_case(D, A, act, tanh, N, T, seed, noise="host", rows=None, top=None, logstd=None, noise_step0=0, ep_cap=64,
                 counters=None, boot=True, publish=7, discount=DISCOUNT, reward_scale=1.0, env=None, head="gauss",
                 cat_seed=0xC011, env_offset=0, head_scale=30.0, ls_bias=-1.5, stress=None, tie=None, peak=None, eps_scale=1.0):
    """Planted inputs of one launch.  noise: "host" (a block of N(0, 1) clipped to +-3), "device" (Philox, keyed
    noise_step0 + t) or "det".  The ring has rows > T and top > 0 so that it wraps inside the launch.
    head: "gauss" (a shared log_std tail), "cat" (A logits, no tail; device or det noise only: the uniform of (cat_seed,
    noise_step0 + t, env_offset + n); the ring's acts are (N, 1), the index) or "sd" (2A head rows [mean | raw log_std], no
    tail) -- the networks are `make_nets`'.  eps_scale: host noise times this (a tanh action under std e^2 saturates)."""
    rs = np.random.RandomState(seed)
    assert head in ("gauss", "cat", "sd") and (head != "cat" or noise in ("device", "det"))
    pf, vf = make_nets(D, A, seed, head, head_scale, ls_bias, stress, tie, peak)
    if head == "cat":
        tanh = False
    rows = T + 3 if rows is None else rows
    top = rows - max(1, T // 2) if top is None else top
    horizon, max_frames = T + 8, T + 4
    t_env, cur_step = plant_counters(N, T, horizon, max_frames) if counters is None else counters(N, T, horizon, max_frames)
    eA, eB = dynamics_matrices(D, A) if env is None else env
    c = dict(D=D, A=A, act=act, tanh=tanh, N=N, T=T, rows=rows, top=top, horizon=horizon, max_frames=max_frames,
             pf=pf, vf=vf, logstd=torch.full((A,), float(np.log(0.125))) if logstd is None else logstd,
             env_A=np.asarray(eA, np.float32), env_B=np.asarray(eB, np.float32), seed_base=int(seed) * N, noise=noise,
             noise_step0=noise_step0, discount=discount, reward_scale=reward_scale, ep_cap=ep_cap, step0=100, boot=boot,
             publish=publish, cur_obs=(0.5 * rs.randn(N, D)).astype(np.float32), t_env=t_env, cur_step=cur_step,
             episode_idx=(np.arange(N) % 3).astype(np.int32), ep_return=(rs.randint(-16, 17, N) / 8.0).astype(np.float32),
             epoch_reward0=12.5, pub_src=rs.randint(0, 2 ** 31 - 1, max(publish, 1)).astype(np.uint32))
    if head != "gauss":
        c.update(head=head, logstd=None, cat_seed=int(cat_seed), env_offset=int(env_offset), eps_scale=float(eps_scale))
    c["eps"] = noise_block(c, T)
    return c


def head_of(c):
    return c.get("head", "gauss")


def acts_width(c):
    """Floats per cell of the ring's acts: the index of a categorical action, else the A action dims."""
    return 1 if head_of(c) == "cat" else c["A"]


def noise_block(c, T, step0=None):
    """(T, N, A) float32: what the launch adds to the means (zeros: deterministic).  Categorical head: (T, N, 1), the
    uniforms `_categorical_ref.uniforms` states for (cat_seed, noise_step0 + t, env_offset + n)."""
    N, A = c["N"], c["A"]
    if head_of(c) == "cat":
        if c["noise"] == "det":
            return np.zeros((T, N, 1), np.float32)
        s0 = c["noise_step0"] if step0 is None else step0
        return CR.uniforms(c["cat_seed"], s0, T, N, c["env_offset"])[..., None].astype(np.float32)
    if c["noise"] == "det":
        return np.zeros((T, N, A), np.float32)
    if c["noise"] == "host":
        return (np.clip(np.random.RandomState(c["seed_base"] + 17 + 1000 * c.get("salt", 0)).randn(T, N, A), -3, 3) *
                c.get("eps_scale", 1.0)).astype(np.float32)
    s0 = c["noise_step0"] if step0 is None else step0
    seeds = np.int64(c["seed_base"]) + np.arange(N, dtype=np.int64)
    return np.stack([philox.normal_vector(A, s0 + t, 0, philox.TAG_NOISE, seeds) for t in range(T)]).astype(np.float32)


def ring_rows(c):
    return [(c["top"] + t) % c["rows"] for t in range(c["T"])]


def continue_case(c, o, T=None):
    """The case of the NEXT launch: env, collector (and normaliser) state as run `o` left them, the ring's top and the noise
    key advanced by the steps taken, fresh noise."""
    D = c["D"]
    c2 = dict(c, cur_obs=np.asarray(o["cur_obs"]).copy(), t_env=np.asarray(o["t_env"]).copy(), cur_step=np.asarray(o["cur_step"]).copy(),
              episode_idx=np.asarray(o["episode_idx"]).copy(), ep_return=np.asarray(o["ep_return"]).copy(),
              epoch_reward0=float(o["epoch_reward"]), top=(c["top"] + c["T"]) % c["rows"], noise_step0=c["noise_step0"] + c["T"],
              salt=c.get("salt", 0) + 1, T=c["T"] if T is None else T)
    if "state" in c:
        s = np.asarray(o["state"])
        c2.update(state=(s[:D].copy(), s[D:2 * D].copy(), float(s[2 * D])), policy_obs=np.asarray(o["policy_obs"]).copy())
    c2["eps"] = noise_block(c2, c2["T"])
    return c2


def step_cases():
    """[(id, kwargs of rollout_case)]: every instantiation at N = 40 x 12 steps; the benchmark shape at every N x T; the
    noise modes; the clamped log_std columns (plain actions: with std e^2 a tanh action saturates)."""
    out = []
    for k, (D, A, act, tanh) in enumerate(INSTANCES):
        out.append(("inst-D%d-A%d-%s-%s" % (D, A, act, "tanh" if tanh else "plain"),
                    dict(D=D, A=A, act=act, tanh=tanh, N=40, T=12, seed=30 + k)))
    for N in ROLL_N:
        for T in ROLL_T:
            out.append(("N%d-T%d" % (N, T), dict(D=17, A=6, act="tanh", tanh=True, N=N, T=T, seed=100 + 13 * N + T)))
    out.append(("wide-N17-T5", dict(D=32, A=8, act="relu", tanh=True, N=17, T=5, seed=61)))
    out.append(("det", dict(D=17, A=6, act="tanh", tanh=True, N=40, T=5, seed=62, noise="det")))
    out.append(("det-rt", dict(D=5, A=3, act="relu", tanh=False, N=17, T=5, seed=63, noise="det")))
    out.append(("epcap", dict(D=17, A=6, act="tanh", tanh=True, N=40, T=12, seed=64, ep_cap=3)))
    out.append(("noboot", dict(D=17, A=6, act="tanh", tanh=True, N=17, T=5, seed=65, boot=False, publish=0)))
    out.append(("scale", dict(D=17, A=6, act="tanh", tanh=True, N=17, T=5, seed=66, reward_scale=5.0, discount=0.9)))
    return out


# ------------------------------------------------------------------ cases of the categorical / state-dependent-std heads
CAT_INSTANCES = [(17, 6, "tanh"), (5, 3, "relu"), (32, 8, "tanh"), (4, 2, "tanh"), (18, 2, "relu"),
                 (17, 5, "relu")]                                  # A = 5: the high lane group holds exactly one action
SD_INSTANCES = [(17, 6, "tanh"), (5, 3, "relu"), (32, 8, "tanh"), (4, 1, "tanh"), (18, 1, "relu"), (18, 8, "relu")]
HEAD_N, HEAD_T = (1, 15, 16, 17), (1, 5)
BORDERLINE_CAP = 0.01                                             # tests/_categorical_rollout_ref.py states the same 1 %
# The stress heads of tests/_gauss_sd_rollout_ref.py::STRESS_CASES on this file's networks: (stress of `make_nets`, the share
# of ALL log_std elements the float64 restatement puts on the upper clamp (min, max), on the lower clamp (min, max)).  The rows
# are scaled by 600 where that file has 300: oracle.nets' head rows are smaller than the policy classes', and at 300 only
# 3 % to 8 % of the elements reach the upper clamp.
SD_STRESS = {"span": (("span", 600.0, 1.0), (0.05, 0.60), (0.0, 0.0)),
             "pinned": (("pinned", 600.0, 0.0), (0.08, 0.40), None),      # lower: exactly the last dim, 1 / A
             "span-tanh": (("span", 600.0, 1.0), (0.05, 0.60), (0.0, 0.0))}      # (run with host noise times 0.1)
# A head whose rows 1 and A - 1 are one float row 45 above the rest: in float32 AND in float64 e_1 = e_{A-1} = 1, every other
# term is below e^-43 and vanishes in the sums, P_1 = ... = P_{A-2} = 1 and S = 2 exactly.  EXACT_CAT_SEED is the first key
# (searched upwards from 0) under which some (t, n) of the 40 x 12 launch draws u = 1/2 exactly, so u S == P_1: the one kind
# of cell on which `>=` and `>` at the threshold differ.
# With head weights times 3000 the logits reach +-30, yet in most cells two of them are within a few units of each other.  Row
# 2's bias + 160 puts one logit at least 100 above the rest everywhere: every other expf is below e^-100 (flushed or
# denormal), S rounds to 1 in float32 and the drawn index is the arg-max for every u.
PEAK_BIAS = 160.0
EXACT_TIE, EXACT_CAT_SEED, EXACT_CELL = 45.0, 38743, (0, 5)      # (the cell (t, n) with u = 1/2; one draw in 2^24 is)
# case id -> seeds skipped: the first seed(s) of these cases put more than BORDERLINE_CAP of the cells within the margin of a
# prefix sum, or (sd) too few tanh rows inside logp_keep (tests/test_rollout_heads_cpu.py asserts both on the seed used)
HEAD_SEED_BUMP = {}


def head_cases():
    """[(id, kwargs of rollout_case)] of tests/test_rollout_heads_*.py: every instantiation of both heads at N = 40 x 12 steps
    with planted counters and a ring that wraps; the (17, 6, tanh) shape at N around the 16-env tile x 1 / 5 steps; the noise
    modes; the categorical keys; ties and peaks; the log_std clamps; the bookkeeping variants."""
    out = []
    cat = lambda **kw: dict(dict(D=17, A=6, act="tanh", tanh=False, N=40, T=12, head="cat", noise="device"), **kw)
    sd = lambda **kw: dict(dict(D=17, A=6, act="tanh", tanh=True, N=40, T=12, head="sd"), **kw)
    for D, A, act in CAT_INSTANCES:
        out.append(("cat-inst-D%d-A%d-%s" % (D, A, act), cat(D=D, A=A, act=act)))
    for D, A, act in SD_INSTANCES:
        out.append(("sd-inst-D%d-A%d-%s" % (D, A, act), sd(D=D, A=A, act=act)))
    out.append(("sd-plain-D17-A6", sd(tanh=False)))
    out.append(("sd-plain-D32-A8", sd(D=32, A=8, tanh=False)))
    for N in HEAD_N:
        for T in HEAD_T:
            out.append(("cat-N%d-T%d" % (N, T), cat(N=N, T=T)))
            out.append(("sd-N%d-T%d" % (N, T), sd(N=N, T=T)))
    out.append(("cat-det", cat(T=5, noise="det")))
    out.append(("sd-det", sd(T=5, noise="det")))
    out.append(("sd-device", sd(T=5, noise="device", noise_step0=7)))
    # the uniform's key: a second rank's shard (not a multiple of 4: the envs straddle Philox blocks differently), and a
    # counter whose high word changes inside the launch
    out.append(("cat-env-offset", cat(T=5, env_offset=1000003)))
    out.append(("cat-high-word", cat(T=5, noise_step0=2 ** 32 - 3)))
    out.append(("cat-tie-det", cat(T=5, noise="det", tie=5.0)))
    out.append(("cat-tie", cat(T=5, tie=5.0)))
    out.append(("cat-peaked", cat(head_scale=3000.0)))
    out.append(("cat-peaked-S1", cat(head_scale=3000.0, peak=PEAK_BIAS)))
    out.append(("cat-exact-threshold", cat(tie=EXACT_TIE, cat_seed=EXACT_CAT_SEED)))
    for shape in ((17, 6), (32, 8)):
        for kind in ("span", "pinned"):
            out.append(("sd-%s-D%d-A%d" % (kind, *shape), sd(D=shape[0], A=shape[1], tanh=False, T=6, stress=SD_STRESS[kind][0])))
    out.append(("sd-span-tanh", sd(T=6, stress=SD_STRESS["span-tanh"][0], eps_scale=0.1)))
    for h, mk in (("cat", cat), ("sd", sd)):
        out.append((h + "-epcap", mk(ep_cap=3)))
        out.append((h + "-noboot", mk(N=17, T=5, boot=False, publish=0)))
        out.append((h + "-scale", mk(N=17, T=5, reward_scale=5.0, discount=0.9)))
    return [(name, dict(kw, seed=500 + 3 * k + HEAD_SEED_BUMP.get(name, 0))) for k, (name, kw) in enumerate(out)]


def two_launch_case(head):
    """Device noise from noise_step0 = 100, continued by `continue_case` over a second launch of 7 steps."""
    kw = dict(D=17, A=6, act="tanh", tanh=head == "sd", N=40, T=5, head=head, noise="device", noise_step0=100, rows=15, top=8)
    return rollout_case(seed=dict(cat=483, sd=484)[head], **kw)


def sd_stress_of(kw):
    """The SD_STRESS entry a case's kwargs were built from, or None."""
    for name, entry in SD_STRESS.items():
        if kw.get("stress") == entry[0]:
            return entry
    return None


def clamp_logstd(A, lower=True):
    """One column at +3 (clamped to 2) and, `lower`, one at -25 (clamped to -20); the rest log(0.125)."""
    ls = torch.full((A,), float(np.log(0.125)))
    ls[A - 1] = 3.0
    if lower:
        ls[0] = -25.0
    return ls


def quiet_counters(N, T, horizon, max_frames):
    """No env ends an episode or runs over its length inside the launch: no marker, the second forward is never taken."""
    return np.zeros(N, np.int32), np.zeros(N, np.int32)


def big_counters(N, T, horizon, max_frames):
    """The large value-pass case: over-length cells in step 2 (first round of tiles) and in the last step (second round),
    on every seventh env; nothing else."""
    t_env, cur = np.zeros(N, np.int32), np.zeros(N, np.int32)
    cur[0::7] = max_frames - 1 - 2
    cur[3::7] = max_frames - 1 - (T - 1)
    return t_env, cur


VALUE_CASES = [  # M = T N: less than one tile; tiles that straddle time rows; exact tiles
    ("M6", dict(D=17, A=6, act="tanh", tanh=True, N=3, T=2, seed=71, publish=5000)),       # (one workgroup copies 5000 words)
    ("M540", dict(D=17, A=6, act="tanh", tanh=True, N=45, T=12, seed=72)),
    ("M80", dict(D=17, A=6, act="relu", tanh=True, N=16, T=5, seed=73)),
    ("M540-wide", dict(D=32, A=8, act="tanh", tanh=True, N=45, T=12, seed=74)),
    ("quiet", dict(D=17, A=6, act="tanh", tanh=True, N=45, T=12, seed=75, counters=quiet_counters)),
    ("noboot", dict(D=17, A=6, act="tanh", tanh=True, N=45, T=12, seed=76, boot=False))]
BIG = dict(D=17, A=6, act="tanh", tanh=True, N=1031, T=33, seed=77, counters=big_counters, ep_cap=8)
VP_TILES_PER_ROUND = 2048                                        # 512 workgroups of 4 waves, one 16-cell tile per wave


def counters_walk(c):
    """The integer side of the launch, exact: per (t, n) done, surpass and the counters BEFORE the step; the counters after
    the launch; the finished episodes [(step, env)] in (step, env) order."""
    N, T = c["N"], c["T"]
    t_env, cur, ep = c["t_env"].astype(np.int64).copy(), c["cur_step"].astype(np.int64).copy(), c["episode_idx"].astype(np.int64).copy()
    done, over, ep_new = np.zeros((T, N), bool), np.zeros((T, N), bool), np.zeros((T, N), np.int64)
    for t in range(T):
        t_env += 1
        cur += 1
        done[t], over[t] = t_env >= c["horizon"], cur >= c["max_frames"]
        flag = done[t] | over[t]
        ep = ep + flag
        ep_new[t] = ep
        t_env[flag], cur[flag] = 0, 0
    return dict(done=done, over=over, flag=done | over, ep_new=ep_new, t_env=t_env.astype(np.int32), cur_step=cur.astype(np.int32),
                episode_idx=ep.astype(np.int32), episodes=[(t, n) for t in range(T) for n in range(N) if done[t, n]])


def reset_draw(c, ep_idx, n):
    """Reset observations of envs `n` entering episode `ep_idx` (Philox, TAG_RESET, keyed by the episode index)."""
    return philox.normal_vector(c["D"], np.asarray(ep_idx, np.int64), 0, philox.TAG_RESET,
                                np.int64(c["seed_base"]) + np.asarray(n, np.int64)).astype(np.float32)


def event_counts(c):
    """What the planted counters guarantee: counts of (t, n) cells per kind, of envs without any event, whether the events
    fall in different steps / different 16-env tiles, and whether some (16-cell) value-pass tile holds marker cells next
    to cells without one."""
    w = counters_walk(c)
    done, over = w["done"], w["over"]
    only_d, only_o, both = done & ~over, over & ~done, done & over
    ev = np.argwhere(w["flag"])
    m = over.reshape(-1)
    pad = (-len(m)) % 16
    tiles = np.concatenate([m, np.zeros(pad, bool)]).reshape(-1, 16)
    size = np.minimum(16, len(m) - 16 * np.arange(len(tiles)))
    return dict(done=int(only_d.sum()), over=int(only_o.sum()), both=int(both.sum()), quiet=int((~w["flag"].any(0)).sum()),
                steps=len(set(ev[:, 0])), tiles=len(set(ev[:, 1] // 16)),
                mixed_tiles=int(((tiles.sum(1) > 0) & (tiles.sum(1) < size)).sum()))


# ------------------------------------------------------------------ one step, teacher-forced
def cat_terms(c, logits, u, acts_stored):
    """The categorical head of one step in float64 from the restated logits l (M, A), the step's uniforms u (M,) and the
    STORED action indices (M, 1): m = max l, e_k = exp(l_k - m), the prefix sums P_k in ascending k, S = P_{A-1}; the action
    is the smallest k with P_k >= u S, else A - 1 (det: arg-max, the lowest index among equal logits).

    Which index a float32 implementation may store.  Its logits are l_k + d_k with |d_k| <= h_k = 1e-5 (1 + |l_k|) (the head
    allowance), H = max_k h_k.  exp(l'_k - m') = e_k exp(d_k) exp(m - m'): relative to float64 every term, hence every prefix
    sum and S, moves by a factor within e^{+-2H} (d_k and the maximum's own shift).  Float32 adds: the subtraction l_k - m
    rounds once, U |l_k - m| in the exponent, a relative U X on the term with X = max_k (m - l_k); expf is within an ulp, 2 U;
    the A additions of the sum round once each, A U of the sum; the product u S rounds once.  So the comparison P'_k >= thr'
    can differ from P_k >= u S only where |P_k - u S| <= margin_k = (P_k + u S) (e^{2H} - 1 + (A + 3 + X) U): such a prefix
    sum is CLOSE and the cell BORDERLINE.  The stored index must be the restated one, or its direct neighbour on the side of
    a close prefix sum: k + 1 where P_k is close (the implementation saw it below the threshold), k - 1 where P_{k-1} is close
    (saw it reach the threshold).  det: the arg-max may move to k where l_k < l_a and l_k >= l_a - h_k - h_a; logits that
    are EQUAL floats in float64 (bit-identical head rows) are equal in any arithmetic, and the lowest index must win.

    log pi at the stored index a, (l_a - m) - log S = l_a - logsumexp(l): the allowance moves it by |d_a| + max |d| <= 2 H.
    Float32: the subtraction U |l_a - m|; S is off by the relative (A - 1) U of the additions + 2 U of expf + A U / e of the
    exponents' roundings (x e^-x <= 1 / e, the largest term is 1 <= S), below (2 A + 2) U, and log S by as much; logf within
    two ulps of |log S| on either side of the result's rounding, 4 U |log S|; the last subtraction U |log pi|:
    b_logp = 2 H + U (|l_a - m| + 4 |log S| + |log pi| + 2 A + 2).

    -> dict: logits, k_want, k_stored (M,), allowed (M, A) bool, border (M,) bool, onehot_want / onehot_stored (M, A), logp,
    b_logp, keep (all rows), S."""
    logits = np.asarray(logits, np.float64)
    M, A = logits.shape
    rows = np.arange(M)
    h = 1e-5 * (1.0 + np.abs(logits))
    H = h.max(1)
    m = logits.max(1, keepdims=True)
    pre = np.cumsum(np.exp(logits - m), axis=1)                    # (a sequential scan per row: ascending k)
    S = pre[:, -1]
    allowed = np.zeros((M, A), bool)
    if c["noise"] == "det":
        want = (logits == m).argmax(1)
        lw, hw = logits[rows, want][:, None], h[rows, want][:, None]
        allowed = (logits < lw) & (logits >= lw - h - hw)
    else:
        thr = (np.asarray(u, np.float64) * S)[:, None]
        hit = pre >= thr
        want = np.where(hit.any(1), hit.argmax(1), A - 1)
        rel = np.expm1(2.0 * H) + (A + 3 + (m - logits).max(1)) * U
        close = np.abs(pre - thr) <= rel[:, None] * (pre + thr)
        up = close[rows, want] & (want < A - 1)
        dn = close[rows, np.maximum(want - 1, 0)] & (want > 0)
        allowed[rows[up], want[up] + 1] = True
        allowed[rows[dn], want[dn] - 1] = True
    border = allowed.any(1)
    allowed[rows, want] = True
    k = np.asarray(acts_stored, np.float64).reshape(M)
    assert np.isfinite(k).all() and (k == np.floor(k)).all() and (k >= 0).all() and (k < A).all(), \
        "a stored categorical action is not an index in [0, A)"
    k = k.astype(np.int64)
    la = logits[rows, k]
    logS = np.log(S)
    lp = (la - m[:, 0]) - logS
    b_lp = 2.0 * H + U * (np.abs(la - m[:, 0]) + 4.0 * np.abs(logS) + np.abs(lp) + 2.0 * A + 2.0)
    eye = np.eye(A)
    return dict(logits=logits, k_want=want, k_stored=k, allowed=allowed, border=border, onehot_want=eye[want], onehot_stored=eye[k],
                logp=lp, b_logp=b_lp, keep=np.ones(M, bool), S=S)


def sd_logp_terms(c, mean, raw, acts, h, h_ls):
    """log pi of a state-dependent-std head at the STORED actions, in float64 per cell: ls = clamp(raw, -20, 2), the terms
    of `_gauss_ref.logp_parts` with one log_std per cell and dim.  Bound per element, `_gauss_ref.logp_bound`'s form
    2 U (4 |quad| + |ls| + |corr| + 1) [+ |zc| 5e-7 / var for tanh actions], and on top of it
      quad (2 + 2 |ls|) 2^-23   1 / var = __expf(-2 ls) is exp2 of a rounded product (`_gauss_ref.act_bound`'s derivation with
                                x = -2 ls; the shared-std head forms it once per launch from a log_std of its own choosing)
      |zc| / var h              the head allowance on the mean
      quad (e^{2 h_ls} - 1) + h_ls   the head allowance on the raw log_std: d(-quad - ls) / d ls = 2 quad - 1
    and A U of the sum of the absolute terms for the A additions.
    Elements ON THE LOWER CLAMP (raw <= -20: var = e^-40, the term is float32 noise of the action divided by e^-40, DESIGN
    section 7) are left out of the sum and of the bound: `low` marks them, and `qmax_low` is the most their quad terms can
    be for a plain action, sum of (2^-23 max(|mean| + h, 1))^2 e^40 / 2 (the stored action is the mean rounded once, `verify`)."""
    tm, tr, ta = torch.from_numpy(mean), torch.from_numpy(raw), torch.from_numpy(np.asarray(acts, np.float64))
    if c["tanh"]:
        ta = ta.clamp(-1 + 1e-12, 1 - 1e-12)
    p = {k: v.numpy() for k, v in G.logp_parts(tm, tr, ta, c["tanh"]).items()}
    quad, ls, corr, zc = np.abs(p["quad"]), np.abs(p["ls"]), np.abs(p["corr"]), np.abs(p["zc"])
    terms = -p["quad"] - p["ls"] - G.HALF_LOG_2PI - p["corr"]
    per = 2.0 * U * (4.0 * quad + ls + corr + 1.0) + quad * (2.0 + 2.0 * ls) * 2.0 * U + zc / p["var"] * h + \
        quad * np.expm1(2.0 * h_ls) + h_ls
    if c["tanh"]:
        per = per + zc * 5e-7 / p["var"]
    low = np.asarray(raw) <= -20.0
    A = mean.shape[1]
    b = (per * ~low).sum(-1) + A * U * ((quad + ls + G.HALF_LOG_2PI + corr) * ~low).sum(-1)
    qmax = 0.5 * np.exp(40.0) * (2.0 ** -23 * np.maximum(np.abs(mean) + h, 1.0)) ** 2
    return dict(logp=(terms * ~low).sum(-1), b_logp=b, keep=G.logp_keep(torch.from_numpy(np.asarray(acts, np.float64)), c["tanh"]).numpy(),
                low=low, qmax_low=(qmax * low).sum(-1))


def step_terms(c, obs_policy, obs_raw, eps, acts_stored=None, lp_cols=None):
    """One step of M cells from given inputs, in float64.  obs_policy (M, D): what the policy sees; obs_raw (M, D): the env's
    state (the same without a normaliser); eps (M, A).  -> dict:
      mean, act, b_act      the action and its bound: `_gauss_ref.act_bound` on top of what a head error of
                            h = 1e-5 (1 + |mean|) moves it by (slope of tanh <= 1)
      next_obs, b_next      tanh(M [obs_raw; a]) with a the STORED action when given (then the action's error does not enter),
                            bound (K + 2) U sum_k |M_k x_k| for the K = D + A term MFMA / fma chain + trl_tanh's 2e-7
                            (+ sum_o |B_o| b_act_o when the restated action is used)
      reward, b_rew         scale (nx0 - 0.1f sum a^2): nx0's bound; the squares, the lane's fma and the four-lane sum
                            (2 + 3 roundings) and the product with 0.1f (1) on 0.1 sum a^2; the subtraction and the scaling
                            (2) on the result
      logp, b_logp          log pi_old at the stored action: `_gauss_ref.logp_bound` + sum_o |zc_o| / var_o h_o (the head
                            allowance enters through the mean).
    head "cat": eps is the step's uniform (M, 1) and acts_stored the stored INDEX (M, 1), required; the env takes the one-hot
    row of the stored index (sum a^2 is exactly 1), b_act is zero and `cat_terms`' keys are added (allowed, border, logp, ...).
    head "sd": mean and raw log_std are the head's two halves; b_act adds what the allowance on the raw log_std moves the
    std by; log pi and its bound are `sd_logp_terms`' (keys low, qmax_low, raw besides)."""
    D, A = c["D"], c["A"]
    x = np.asarray(obs_policy, np.float64)
    extra = {}
    if head_of(c) == "cat":
        assert acts_stored is not None and lp_cols is None
        extra = cat_terms(c, mlp(c["pf"], x, c["act"]), np.asarray(eps, np.float64)[:, 0], acts_stored)
        mean, act, b_act = extra["logits"], extra["onehot_want"], np.zeros((len(x), A))
        acts_stored = extra.pop("onehot_stored")
    elif head_of(c) == "sd":
        head = mlp(c["pf"], x, c["act"])
        mean, raw = head[:, :A], head[:, A:]
        tm, te, ls = torch.from_numpy(mean), torch.from_numpy(np.asarray(eps, np.float64)), torch.from_numpy(raw)
        act = G.explore(tm, ls, te, c["tanh"])[0].numpy()
        h, h_ls = 1e-5 * (1.0 + np.abs(mean)), 1e-5 * (1.0 + np.abs(raw))
        # a raw log_std off by h_ls moves the std by the relative amount e^h_ls - 1 (the clamp is 1-Lipschitz: no more on
        # an element near an edge), the pre-activation by std |eps| times that, the action by no more (slope of tanh <= 1)
        b_act = h + G.act_bound(tm, ls, te, c["tanh"]).numpy() + \
            np.exp(np.clip(raw, -20.0, 2.0)) * np.abs(np.asarray(eps, np.float64)) * np.expm1(h_ls)
        extra = dict(raw=raw, h_ls=h_ls)
    else:
        mean = mlp(c["pf"], x, c["act"])
        tm, te, ls = torch.from_numpy(mean), torch.from_numpy(np.asarray(eps, np.float64)), c["logstd"].double()
        act = G.explore(tm, ls, te, c["tanh"])[0].numpy()
        h = 1e-5 * (1.0 + np.abs(mean))
        b_act = h + G.act_bound(tm, ls, te, c["tanh"]).numpy()
    a_env = act if acts_stored is None else np.asarray(acts_stored, np.float64)
    eA, eB = c["env_A"].astype(np.float64), c["env_B"].astype(np.float64)
    xr = np.asarray(obs_raw, np.float64)
    pre = xr @ eA + a_env @ eB
    mag = np.abs(xr) @ np.abs(eA) + np.abs(a_env) @ np.abs(eB)
    nxt = np.tanh(pre)
    b_next = (D + A + 2) * U * mag + 2e-7 + (b_act @ np.abs(eB) if acts_stored is None else 0.0)
    asq = (a_env * a_env).sum(-1)
    scale = F32(c["reward_scale"])
    raw = nxt[:, 0] - F32(0.1) * asq
    rew = scale * raw
    b_rew = scale * (b_next[:, 0] + U * (6.0 * F32(0.1) * asq + 2.0 * np.abs(raw))) + \
        (0.0 if acts_stored is not None else scale * 0.2 * (np.abs(a_env) * b_act).sum(-1))
    out = dict(mean=mean, act=act, b_act=b_act, next_obs=nxt, b_next=b_next, reward=rew, b_rew=b_rew)
    if head_of(c) == "cat":
        out.update(extra)
    elif head_of(c) == "sd":
        out.update(extra)
        if acts_stored is not None:
            out.update(sd_logp_terms(c, mean, extra["raw"], a_env, h, extra["h_ls"]))
    elif acts_stored is not None:
        cols = list(range(A)) if lp_cols is None else list(lp_cols)      # (the action dims log pi is summed over)
        ta = torch.from_numpy(a_env)
        if c["tanh"]:
            ta = ta.clamp(-1 + 1e-12, 1 - 1e-12)
        tm, ls, ta, th = tm[:, cols], ls[cols], ta[:, cols], torch.from_numpy(h)[:, cols]
        p = G.logp_parts(tm, ls, ta, c["tanh"])
        out["logp"] = G.logp(tm, ls, ta, c["tanh"]).numpy()
        out["b_logp"] = (G.logp_bound(tm, ls, ta, c["tanh"]) + (p["zc"].abs() / p["var"] * th).sum(-1)).numpy()
        out["keep"] = G.logp_keep(torch.from_numpy(a_env), c["tanh"]).numpy()
    return out


def values_and_boot(c, obs, next_obs, over):
    """The value pass on (T, N, D) stored observations: V(obs), V(next_obs), their bound 1e-5 (1 + |v|), and the bootstrap
    discount V(next_obs) on the over-length cells with its bound (V's bound, the product's and the sum's rounding are added
    by the caller, who knows the stored reward)."""
    T, N, D = obs.shape
    v = mlp(c["vf"], obs.reshape(-1, D), c["act"])[:, 0].reshape(T, N)
    v2 = mlp(c["vf"], next_obs.reshape(-1, D), c["act"])[:, 0].reshape(T, N)
    return dict(v=v, b_v=1e-5 * (1.0 + np.abs(v)), v2=v2, b_v2=1e-5 * (1.0 + np.abs(v2)),
                bootstrap=F32(c["discount"]) * v2 * over)


# ------------------------------------------------------------------ a whole launch on the CPU
PERTURBATIONS = (  # named wrong variants of `emulate`: what tests/test_rollout_heads_cpu.py shows `verify` to catch
    "cat_prefix_descending", "cat_gt_threshold", "cat_argmax_last", "cat_no_log_S", "cat_uniform_one_step_late",
    "cat_no_env_offset", "cat_counter_32_bits", "sd_std_unclamped", "sd_log_std_row_o", "sd_exp_minus_ls", "sd_no_tanh_correction",
    "cat_acts_one_hot")


def _cat_draw(c, lg, u, perturb):
    """The categorical head's draw in the dtype of the logits `lg` (N, A): -> (index (N,) int64, log pi (N,))."""
    A = lg.shape[1]
    m = lg.max(dim=-1, keepdim=True)[0]
    e = torch.exp(lg - m)
    S = torch.cumsum(e, dim=-1)[:, -1:]
    if c["noise"] == "det":
        first = (lg == m).to(torch.int64).argmax(dim=-1)
        k = A - 1 - (lg == m).flip(-1).to(torch.int64).argmax(dim=-1) if perturb == "cat_argmax_last" else first
    else:
        thr = torch.as_tensor(u, dtype=lg.dtype).reshape(-1, 1) * S
        if perturb == "cat_prefix_descending":                        # the sums from k = A - 1 down, the first to reach thr
            hit = torch.cumsum(e.flip(-1), dim=-1) >= thr
            k = torch.where(hit.any(-1), A - 1 - hit.to(torch.int64).argmax(dim=-1), torch.zeros(len(lg), dtype=torch.int64))
        else:
            pre = torch.cumsum(e, dim=-1)
            hit = (pre > thr) if perturb == "cat_gt_threshold" else (pre >= thr)
            k = torch.where(hit.any(-1), hit.to(torch.int64).argmax(dim=-1), torch.full((len(lg),), A - 1))
    lp = lg.gather(1, k[:, None]) - m
    if perturb != "cat_no_log_S":
        lp = lp - torch.log(S)
    return k, lp[:, 0]


def _sd_draw(c, head, eps, perturb):
    """The state-dependent-std head's draw in the dtype of `head` (N, 2A): -> (action (N, A), log pi (N,))."""
    A = c["A"]
    mean, raw = head[:, :A], (head[:, :A] if perturb == "sd_log_std_row_o" else head[:, A:])
    ls = raw.clamp(-20.0, 2.0)
    z = mean + torch.exp(raw if perturb == "sd_std_unclamped" else ls) * eps
    act = torch.tanh(z) if c["tanh"] else z
    pre, corr = act, torch.zeros_like(act)
    if c["tanh"]:
        pre = 0.5 * torch.log((1.0 + act) / (1.0 - act))
        if perturb != "sd_no_tanh_correction":
            corr = torch.log((1.0 - act) * (1.0 + act) + 1e-6)
    zc = pre - mean
    iv = torch.exp(-ls) if perturb == "sd_exp_minus_ls" else torch.exp(-2.0 * ls)
    return act, (-(zc * zc) * 0.5 * iv - ls - G.HALF_LOG_2PI - corr).sum(-1)


def _perturbed_uniforms(c, perturb):
    """The (T, N, 1) uniforms of a wrongly keyed categorical draw."""
    s0, off = c["noise_step0"], c["env_offset"]
    if perturb == "cat_uniform_one_step_late":
        s0 += 1
    if perturb == "cat_no_env_offset":
        off = 0
    steps = [s0 + t for t in range(c["T"])]
    if perturb == "cat_counter_32_bits":
        steps = [s & 0xFFFFFFFF for s in steps]
    return np.stack([CR.uniforms(c["cat_seed"], s, 1, c["N"], off)[0] for s in steps])[..., None].astype(np.float32)


def emulate(c, dtype=np.float32, cells=None, perturb=None):
    """The launch on the CPU in `dtype`, step after step: -> the RUN dict the GPU file reads back.  Used by the CPU twin: in
    float64 against the oracle's collector, in float32 against every bound of `verify`.  perturb: one of PERTURBATIONS, a
    subtly wrong implementation of a categorical / state-dependent-std head."""
    N, T, D, A, rows = c["N"], c["T"], c["D"], c["A"], c["rows"]
    td = torch.float32 if dtype == np.float32 else torch.float64
    head = head_of(c)
    assert perturb is None or (perturb in PERTURBATIONS and perturb.split("_")[0] == head)
    ring = {k: np.full((rows, N, f), SENT, np.float32 if dtype == np.float32 else np.float64)
            for k, f in (("obs", D), ("next_obs", D), ("acts", acts_width(c)), ("values", 1), ("rewards", 1), ("terminals", 1),
                         ("time_limits", 1), ("old_logp", 1))}
    w = counters_walk(c)
    ob = c["cur_obs"].astype(dtype)
    ep_ret = c["ep_return"].astype(dtype)
    eA, eB = c["env_A"].astype(dtype), c["env_B"].astype(dtype)
    log, epoch, boot = [], float(c["epoch_reward0"]), None
    ls = None if c["logstd"] is None else c["logstd"].to(td)
    eps = c["eps"]
    if head == "cat" and c["noise"] != "det" and perturb in ("cat_uniform_one_step_late", "cat_no_env_offset", "cat_counter_32_bits"):
        eps = _perturbed_uniforms(c, perturb)
    for t, row in enumerate(ring_rows(c)):
        mean = torch.from_numpy(mlp(c["pf"], ob, c["act"], dtype))
        if head == "cat":
            k, lp = _cat_draw(c, mean, eps[t][:, 0].astype(dtype), perturb)
            act = torch.nn.functional.one_hot(k, A).to(td)
            stored_act = (act[:, :1] if perturb == "cat_acts_one_hot" else k[:, None].to(td)).numpy()
        elif head == "sd":
            act, lp = _sd_draw(c, mean, torch.from_numpy(eps[t].astype(dtype)), perturb)
            stored_act = act.numpy()
        else:
            act, lp = G.explore(mean, ls, torch.from_numpy(c["eps"][t].astype(dtype)), c["tanh"])
            stored_act = act.numpy()
        act = act.numpy()
        nxt = np.tanh((ob @ eA + act @ eB).astype(dtype)).astype(dtype)
        raw = (dtype(c["reward_scale"]) * (nxt[:, 0] - dtype(np.float32(0.1)) * (act * act).sum(-1, dtype=dtype))).astype(dtype)
        epoch += float(raw.astype(np.float64).sum())
        ep_ret = (ep_ret + raw).astype(dtype)
        for n in np.nonzero(w["done"][t])[0]:
            log.append((float(c["step0"] + t), float(n), float(ep_ret[n])))
        ep_ret[w["done"][t]] = 0
        v = mlp(c["vf"], ob, c["act"], dtype)[:, 0]
        v2 = mlp(c["vf"], nxt, c["act"], dtype)[:, 0]
        stored = np.where(w["over"][t], (raw + dtype(np.float32(c["discount"])) * v2).astype(dtype), raw)
        for k, val in (("obs", ob), ("next_obs", nxt), ("acts", stored_act), ("values", v[:, None]), ("rewards", stored[:, None]),
                       ("terminals", w["flag"][t][:, None]), ("time_limits", w["done"][t][:, None]),
                       ("old_logp", lp.numpy()[:, None])):
            ring[k][row] = val
        if t == T - 1:
            boot = v2.copy()
        ob = nxt.copy()
        fl = np.nonzero(w["flag"][t])[0]
        if len(fl):
            ob[fl] = reset_draw(c, w["ep_new"][t][fl], fl).astype(dtype)
    ep_log = np.full((c["ep_cap"] + 4, 3), SENT, np.float32)
    for k, e in enumerate(log[:c["ep_cap"]]):
        ep_log[k] = e
    out = dict(ring, cur_obs=ob, t_env=w["t_env"], cur_step=w["cur_step"], episode_idx=w["episode_idx"], ep_return=ep_ret,
               epoch_reward=epoch, ep_count=len(log), ep_log=ep_log, boot=boot if c["boot"] else None,
               pub_dst=c["pub_src"][:c["publish"]].copy())
    return out


# ------------------------------------------------------------------ a launch against the restatement
def _ratio(got, want, bound):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.isfinite(got).all(), "non-finite output"
    return float((np.abs(got - want) / bound).max()) if got.size else 0.0


def verify(c, o, lower_clamp_col=None):
    """-> {quantity: worst err / bound} of run `o` of case `c`; asserts what is exact (flags, counters, bit identities of the
    chain, untouched ring rows, the episode log's (step, env) fields, the publish copy).  Keys that begin with "_" are no
    ratios: the share of borderline cells and the number of moved actions of a categorical run (whose stored indices are
    asserted to be the restated ones or their neighbours, `cat_terms`), the shares of log_std elements on each clamp and of rows
    inside logp_keep of a state-dependent-std run."""
    N, T, D, A = c["N"], c["T"], c["D"], c["A"]
    rr, w = ring_rows(c), counters_walk(c)
    g = {k: np.asarray(o[k])[rr] for k in ("obs", "next_obs", "acts", "values", "rewards", "terminals", "time_limits", "old_logp")}
    for k in g:                                                       # rows outside the launch keep their pre-fill
        rest = np.delete(np.asarray(o[k]), rr, axis=0)
        assert (rest == np.float32(SENT)).all(), k + ": a ring row outside the launch was written"
    M = T * N
    lp_cols = None if lower_clamp_col is None else [o_ for o_ in range(A) if o_ != lower_clamp_col]
    head, AW = head_of(c), acts_width(c)
    st = step_terms(c, g["obs"].reshape(M, D), g["obs"].reshape(M, D), c["eps"].reshape(M, -1), g["acts"].reshape(M, AW), lp_cols)
    res = {}
    if head == "cat":
        # exact on every cell that is not borderline; on a borderline one the restated index or the neighbour on the side of
        # the close prefix sum (`cat_terms`).  Everything below is restated from the STORED index: no cell is left out.
        ok = st["allowed"][np.arange(M), st["k_stored"]]
        assert ok.all(), "%d stored actions are neither the restated index nor its neighbour across a close prefix sum; " \
            "first (t, n) %s: stored %d, restated %d" % ((~ok).sum(), divmod(int(np.nonzero(~ok)[0][0]), N),
                                                         st["k_stored"][~ok][0], st["k_want"][~ok][0])
        res["_share_borderline"] = float(st["border"].mean())
        res["_moved"] = float((st["k_stored"] != st["k_want"]).sum())
    else:
        res["act"] = _ratio(g["acts"].reshape(M, A), st["act"], st["b_act"])
    res["next_obs"] = _ratio(g["next_obs"].reshape(M, D), st["next_obs"], st["b_next"])
    # exact keys
    assert np.array_equal(g["terminals"][..., 0], w["flag"].astype(np.float32)), "terminals"
    assert np.array_equal(g["time_limits"][..., 0], w["done"].astype(np.float32)), "time_limits"
    # the chain: obs[t + 1] is next_obs[t] bit for bit, or the reset draw; cur_obs continues the last row
    follow = np.concatenate([g["obs"][1:], np.asarray(o["cur_obs"])[None]], 0)
    keep = ~w["flag"]
    assert np.array_equal(follow[keep], g["next_obs"][keep]), "obs[t + 1] != next_obs[t] on an env that was not reset"
    tt, nn = np.nonzero(w["flag"])
    if len(tt):
        res["reset"] = _ratio(follow[tt, nn], reset_draw(c, w["ep_new"][tt, nn], nn), RESET_ATOL)
    assert np.array_equal(g["obs"][0], c["cur_obs"]), "obs[0] != cur_obs of the launch"
    for k in ("t_env", "cur_step", "episode_idx"):
        assert np.array_equal(np.asarray(o[k]), w[k]), k
    # values, bootstrap, boot
    vb = values_and_boot(c, g["obs"].astype(np.float64), g["next_obs"].astype(np.float64), w["over"])
    res["values"] = _ratio(g["values"][..., 0], vb["v"], vb["b_v"])
    raw64, b_raw = st["reward"].reshape(T, N), st["b_rew"].reshape(T, N)
    disc = F32(c["discount"])
    want_r = raw64 + vb["bootstrap"]
    b_r = b_raw + w["over"] * (disc * vb["b_v2"] + U * (np.abs(disc * vb["v2"]) + np.abs(want_r)))
    res["rewards"] = _ratio(g["rewards"][..., 0], want_r, b_r)
    if o.get("boot") is not None:
        res["boot"] = _ratio(np.asarray(o["boot"]).reshape(N), vb["v2"][T - 1], vb["b_v2"][T - 1])
    # log pi_old at the stored action
    keepl = st["keep"]
    lp = g["old_logp"].reshape(M)
    assert np.isfinite(lp).all()
    if head == "sd":
        low, lowrow = st["low"], st["low"].any(1)
        res["_share_hi"], res["_share_lo"] = float((st["raw"] >= 2.0).mean()), float(low.mean())
        res["_share_keep"] = float(keepl.mean())
        assert keepl.mean() >= 0.25, "too few rows inside logp_keep"
        full = keepl & ~lowrow
        if full.any():
            res["logp"] = _ratio(lp[full], st["logp"][full], st["b_logp"][full])
        if lowrow.any():
            # Elements on the lower clamp, as `lower_clamp_col` below: std = e^-20 is far below an ulp of the mean, the stored
            # plain action is the mean rounded once, so each such term is -quad + 20 - log(2 pi) / 2 with 0 <= quad <= its share
            # of `qmax_low`; without the clamp it is at least 5 more at quad = 0 and below -1e4 otherwise.
            assert not c["tanh"]
            col = (lp - st["logp"]) - low.sum(1) * (20.0 - G.HALF_LOG_2PI)
            # (1 + 1e-5: __expf(40) is within 42 2^-23 = 5e-6 of e^40, `sd_logp_terms`)
            good = (col <= st["b_logp"] + 1e-3) & (col >= -st["qmax_low"] * (1.0 + 1e-5) - st["b_logp"] - 1e-3)
            assert good[lowrow].all(), "the lower clamp of log_std is not applied"
    elif lower_clamp_col is None:
        assert keepl.mean() >= 0.25, "too few rows inside logp_keep"
        res["logp"] = _ratio(lp[keepl], st["logp"][keepl], st["b_logp"][keepl])
    else:
        # A column whose raw log_std is below -20: std = e^-20 is far below an ulp of the mean, the stored action is the
        # rounded mean and zc is 0 or an ulp or two of it (<= 1.2e-7 for |mean| <= 1), so the column's term of log pi is
        # -quad + 20 - log(2 pi) / 2 with 0 <= quad <= (1.2e-7)^2 / (2 e^-40) = 1.7e3.  Without the clamp the term is 5
        # more at quad = 0 and below -1e4 otherwise.
        assert not c["tanh"]
        col = (lp - st["logp"]) - (20.0 - G.HALF_LOG_2PI)
        assert (col <= st["b_logp"] + 1e-3).all() and (col >= -1.7e3 - 1e-3).all(), "the lower clamp of log_std is not applied"
    # epoch reward: the double sum of the raw rewards (recovered on bootstrapped rows)
    raw_rec = np.where(w["over"], g["rewards"][..., 0].astype(np.float64) - vb["bootstrap"], g["rewards"][..., 0].astype(np.float64))
    b_rec = np.where(w["over"], disc * vb["b_v2"] + U * (np.abs(disc * vb["v2"]) + np.abs(want_r)), 0.0)
    b_epoch = M * 2.0 ** -53 * (np.abs(raw_rec).sum() + abs(c["epoch_reward0"])) + b_rec.sum() + 1e-300
    res["epoch_reward"] = abs(float(o["epoch_reward"]) - (c["epoch_reward0"] + raw_rec.sum())) / b_epoch
    # running returns: float32 sums in step order; the episode log
    run = c["ep_return"].astype(np.float32).copy()
    b_run = np.zeros(N)
    want_log = []
    for t in range(T):
        r32 = np.where(w["over"][t], raw64[t], raw_rec[t]).astype(np.float32)
        run = (run + r32).astype(np.float32)
        b_run = b_run + np.where(w["over"][t], b_raw[t] + U * np.abs(raw64[t]), 0.0) + U * np.abs(run)
        for n in np.nonzero(w["done"][t])[0]:
            want_log.append((c["step0"] + t, n, float(run[n]), b_run[n] + 1e-30))
        run[w["done"][t]], b_run[w["done"][t]] = 0.0, 0.0
    res["ep_return"] = _ratio(np.asarray(o["ep_return"]), run, b_run + 1e-30)
    assert int(o["ep_count"]) == len(want_log), "ep_count %d, %d episodes finished" % (int(o["ep_count"]), len(want_log))
    log = np.asarray(o["ep_log"])
    n_log = min(len(want_log), c["ep_cap"])
    assert (log[n_log:] == np.float32(SENT)).all(), "the episode log was written past its count / cap"
    got_log = log[:n_log][np.lexsort((log[:n_log, 1], log[:n_log, 0]))]
    by_key = {(s, n): (r, b) for s, n, r, b in want_log}
    keys = [(int(s), int(n)) for s, n in got_log[:, :2]]
    assert len(set(keys)) == n_log and all(k in by_key for k in keys), "episode log: wrong (step, env) entries"
    if n_log == len(want_log):
        assert keys == [(s, n) for s, n, _, _ in want_log]
    if n_log:
        res["ep_log"] = max(abs(float(got_log[k, 2]) - by_key[keys[k]][0]) / by_key[keys[k]][1] for k in range(n_log))
    if c["publish"]:
        assert np.array_equal(np.asarray(o["pub_dst"]), c["pub_src"][:c["publish"]]), "publish copy"
    return res


# ------------------------------------------------------------------ the cooperative normalised rollout, one step
def norm_case(act, N, seed, level="centred", clip=10.0, update=1, partial_reset=0, reset_env=None, warm=True):
    """One n_steps = 1 launch of the 17 / 64 / 6 normalised instantiation from planted raw observations, policy observations
    and normaliser state.  level: "centred" (0.5 N(0, 1), the synthetic env's own matrices), "offset" (0.9 +- 1e-2, env_A =
    atanh(0.9) / 0.9 I: the fixed point) or "basin" (+0.995 in every feature, env_A = 3 I: every env in one tanh basin), the
    last two with env_B = 0.05.  reset_env: that env ends its episode in this step (horizon out of reach for all others).
    The state is warmed on one batch of the same distribution."""
    D, A = 17, 6
    rs = np.random.RandomState(seed)
    env = None
    if level != "centred":
        k = 3.0 if level == "basin" else float(np.arctanh(0.9) / 0.9)
        env = (k * np.eye(D, dtype=np.float32), np.full((A, D), 0.05, np.float32))
    c = rollout_case(D, A, act, True, N, 1, seed, noise="host", rows=3, top=2, env=env, boot=False, publish=0)
    c.update(horizon=1 << 20, max_frames=1 << 20, t_env=np.zeros(N, np.int32), cur_step=np.zeros(N, np.int32), level=level,
             norm_clip=clip, norm_update=update, partial_reset=partial_reset, reset_env=reset_env)
    if level == "offset":
        c["cur_obs"] = (0.9 + 1e-2 * rs.randn(N, D)).astype(np.float32)
    elif level == "basin":
        c["cur_obs"] = np.full((N, D), 0.995, np.float32)
    if reset_env is not None:
        c["t_env"][reset_env] = c["horizon"] - 1
    # the distribution the state is warmed on: one step from these observations with actions tanh(0.3 N(0, 1))
    x = np.tanh(c["cur_obs"].astype(np.float64) @ c["env_A"].astype(np.float64) +
                np.tanh(0.3 * rs.randn(max(N, 64), A))[:N] @ c["env_B"].astype(np.float64))
    c["state"] = G.norm_warm_state(x) if warm else G.norm_init(D)
    c["policy_obs"] = G.norm_filt(c["state"], c["cur_obs"], clip).astype(np.float32)
    return c


def parent_moments(x):
    """What the kernel formed before its fix: float32 sums of x and x * x over each 16-env tile (rotating adds: a binary
    tree), widened, added over the tiles in double -> (sum x, sum x^2)."""
    x = np.asarray(x, np.float32)
    N, D = x.shape
    s, q = np.zeros(D), np.zeros(D)
    for lo in range(0, N, 16):
        a = np.zeros((16, D), np.float32)
        a[:len(x[lo:lo + 16])] = x[lo:lo + 16]
        b = (a * a).astype(np.float32)
        for half in (8, 4, 2, 1):
            a = (a[:half] + a[half:2 * half]).astype(np.float32)
            b = (b[:half] + b[half:2 * half]).astype(np.float32)
        s, q = s + a[0].astype(np.float64), q + b[0].astype(np.float64)
    return s, q


def norm_update_parent(state, x):
    mean, var, count = state
    bn = np.asarray(x).shape[0]
    s, q = parent_moments(x)
    bmean = s / bn
    bvar, delta, tot = np.maximum(q / bn - bmean * bmean, 0.0), bmean - mean, count + bn
    return mean + delta * bn / tot, (var * count + bvar * bn + delta * delta * count * bn / tot) / tot, tot


def norm_update_fixed(state, x):
    """The kernel's arithmetic after the fix: d = x - mean in double, 16-env tree sums of d and d^2, tiles added in turn."""
    mean, var, count = state
    d = np.asarray(x, np.float64) - mean
    N, D = d.shape
    s, q = np.zeros(D), np.zeros(D)
    for lo in range(0, N, 16):
        a = np.zeros((16, D))
        a[:len(d[lo:lo + 16])] = d[lo:lo + 16]
        b = a * a
        for half in (8, 4, 2, 1):
            a, b = a[:half] + a[half:2 * half], b[:half] + b[half:2 * half]
        s, q = s + a[0], q + b[0]
    delta, tot = s / N, count + N
    bvar = np.maximum(q / N - delta * delta, 0.0)
    return mean + delta * N / tot, (var * count + bvar * N + delta * delta * count * N / tot) / tot, tot


def state_errors(got, want):
    """(mean, variance) worst relative error of a (mean, var, count) state against `want`; the count must be equal."""
    assert float(got[2]) == float(want[2]), "count"
    return (float((np.abs(got[0] - want[0]) / np.abs(want[0])).max()), float((np.abs(got[1] - want[1]) / want[1]).max()))


def verify_norm_step(c, o):
    """One normalised step against the restatement.  `o`: the ring row (obs, next_obs, acts), cur_obs, policy_obs and state
    after the launch.  -> ratios: act, raw next observation, state (tolerance rel 1e-11 on mean and variance -- the warm
    shard-pair row of tests/test_gauss_collector_kernels_gpu.py -- plus, with a reset env, its restated row's bound
    propagated: 1 / N of the batch), stored next_obs and policy_obs (rtol 2e-7 + atol 1e-7 of the filtered output)."""
    N, D, A, clip = c["N"], c["D"], c["A"], c["norm_clip"]
    row = c["top"]
    obs, nxt, acts = (np.asarray(o[k])[row] for k in ("obs", "next_obs", "acts"))
    assert np.array_equal(obs, c["policy_obs"]), "stored obs is not the policy observation of the launch"
    st = step_terms(c, c["policy_obs"], c["cur_obs"], c["eps"][0], acts)
    res = dict(act=_ratio(acts, st["act"], st["b_act"]))
    reset = np.zeros(N, bool)
    if c["reset_env"] is not None:
        reset[c["reset_env"]] = True
    cur = np.asarray(o["cur_obs"])
    res["raw_next"] = _ratio(cur[~reset], st["next_obs"][~reset], st["b_next"][~reset])
    if reset.any():
        n = np.nonzero(reset)[0]
        res["reset"] = _ratio(cur[n], reset_draw(c, c["episode_idx"][n] + 1, n), RESET_ATOL)
    x = np.where(reset[:, None], st["next_obs"], cur.astype(np.float64))        # the batch the statistics pool
    bx = np.where(reset[:, None], st["b_next"], 0.0)
    got = (np.asarray(o["state"][:D]), np.asarray(o["state"][D:2 * D]), float(o["state"][2 * D]))
    if not c["norm_update"]:
        assert np.array_equal(np.asarray(o["state"]), G.norm_state_vec(c["state"])), "norm_update = 0 changed the state"
        new = c["state"]
    else:
        new = G.norm_update(c["state"], x)
        assert got[2] == new[2], "count"
        # d mean <= sum b / tot; d var <= 2 sum |x - mean| b / tot (first order)
        tot = new[2]
        b_mean = G.NORM_STATE_RTOL * np.abs(new[0]) + bx.sum(0) / tot
        b_var = G.NORM_STATE_RTOL * new[1] + 2.0 * (np.abs(x - new[0]) * bx).sum(0) / tot
        res["state_mean"], res["state_var"] = _ratio(got[0], new[0], b_mean), _ratio(got[1], new[1], b_var)
    wo = G.norm_filt(got, x, clip)                                               # the kernel's own new state filters
    b_out = G.NORM_OUT_ATOL + G.NORM_OUT_RTOL * np.abs(wo) + bx / (np.sqrt(got[1]) + 1e-4)
    res["next_obs"] = _ratio(nxt, wo, b_out)
    res["_share_clamped"] = float((np.abs(nxt) == np.float32(clip)).mean())      # (a share, not a ratio: callers pop it)
    # The policy's next input.  The reset flag is over ALL envs when the statistics are updated (the workgroups meet); with
    # frozen statistics it is the 16-env tile's own.  Flagged envs: raw observations (reset draws included), or with
    # normalize_partial_reset their filtered ones; the others: the stored (normalised) next observation, bit for bit.
    pol = np.asarray(o["policy_obs"])
    tile = np.arange(N) // 16
    flagged = np.full(N, reset.any()) if c["norm_update"] else np.isin(tile, tile[reset])
    assert np.array_equal(pol[~flagged], nxt[~flagged]), "no reset in sight: the policy sees the stored next observation"
    if not c["partial_reset"]:
        assert np.array_equal(pol[flagged], cur[flagged]), "an env was reset: the policy's input is the raw observation"
    elif flagged.any():
        wp = G.norm_filt(got, cur[flagged], clip)
        res["policy_obs"] = _ratio(pol[flagged], wp, G.NORM_OUT_ATOL + G.NORM_OUT_RTOL * np.abs(wp))
        assert np.array_equal(pol[flagged & ~reset], nxt[flagged & ~reset]), "filtering an env that was not reset changed it"
    return res


# ------------------------------------------------------------------ GAE / discounted return
GAE_T, GAE_N = (1, 2, 63, 64, 65, 255, 256, 257, 513, 700), (1, 7, 8, 9, 100, 136)
GAE_SHAPES = sorted({(T, N) for T in GAE_T for N in (9, 100)} | {(257, N) for N in GAE_N})
K_STEP, K_TREE = 4, 14


def gae_case(T, N, seed, gamma=0.99, tau=0.95, plain=False):
    """Random rewards / values, terminals with probability 0.03 (half of them time limits), and planted envs (N >= 7; with
    fewer, as many as fit): 0 terminal at T - 1, 1 at T - 256, 2 at T - 257 (both sides of the chunk carry; each with tl),
    3 terminal at T - 256 without tl, 4 no terminal at all, 5 terminal at every step (tl on the even ones), 6 last_terminal
    set.  plain: no terminals at all (gamma = tau = 1 growth case)."""
    rs = np.random.RandomState(seed)
    r, v = rs.randn(T, N).astype(np.float32), rs.randn(T, N).astype(np.float32)
    d = rs.rand(T, N) < (0.0 if plain else 0.03)
    tl = d & (rs.rand(T, N) < 0.5)
    lv, lt = rs.randn(N).astype(np.float32), (rs.rand(N) < 0.3)
    planted = {}
    if not plain:
        def put(n, t, with_tl):
            if n < N and 0 <= t < T:
                d[t, n], tl[t, n] = True, with_tl
                planted.setdefault(n, []).append(t)
        put(0, T - 1, True), put(1, T - 256, True), put(2, T - 257, True), put(3, T - 256, False)
        if N > 4:
            d[:, 4], tl[:, 4], lt[4] = False, False, False
        if N > 5:
            d[:, 5] = True
            tl[:, 5] = (np.arange(T) % 2 == 0)
        if N > 6:
            lt[6] = True
    return dict(T=T, N=N, r=r, v=v, d=d.astype(np.float32), tl=tl.astype(np.float32), lv=lv, lt=lt.astype(np.float32),
                gamma=gamma, tau=tau, planted=planted)


def _scan_bound(abar, c, v, y, T, carry_mag):
    """E_t = |c_t| E_{t+1} + K_STEP U (abar_t + |c_t| Y_{t+1}), Y_t = abar_t + |c_t| Y_{t+1} the recurrence of magnitudes
    (Y_T = |carry|, E_T = 0: the carry is an input); + K_TREE U Y_t per T_CHUNK crossed on the way from T (the lane
    composition and the chunk carry: 7 compositions of two roundings each on a term's path); + U (|y_t| + |v_t|) for the
    second output, y +- v."""
    E, Y = np.zeros_like(carry_mag), carry_mag.astype(np.float64)
    out = np.zeros_like(abar)
    for t in range(T - 1, -1, -1):
        E = np.abs(c[t]) * E + K_STEP * U * (abar[t] + np.abs(c[t]) * Y)
        Y = abar[t] + np.abs(c[t]) * Y
        chunks = (T - 1 - t) // 256 + 1
        out[t] = E + K_TREE * U * Y * chunks + U * (np.abs(y[t]) + np.abs(v[t]))
    return out


def gae_ref(g, filt, use_lt):
    """(adv, ret, bound) of trl_gae_f32: oracle.replay.gae with the float32 gamma and tau the kernel is handed, and the bound
    recurrence.  Forming a = (r + nd gamma v' - v) f rounds three times on terms of size abar = |r| + |gamma v'| + |v| (not
    on |a|: the terms cancel), c = nd gamma tau f once, one composition y = a + c y' twice: K_STEP = 4 on abar (3 + the
    sum) and >= 3 on |c| Y."""
    T, N = g["T"], g["N"]
    gam, tau = F32(g["gamma"]), F32(g["tau"])
    lv = g["lv"].astype(np.float64) * (1.0 - g["lt"] if use_lt else 1.0)
    sh = lambda x: np.asarray(x, np.float64)[..., None]
    adv, ret = replay.gae(sh(g["r"]), sh(g["v"]), sh(g["d"]), sh(g["tl"]), lv[:, None], gam, tau, bool(filt))
    r, v, d, tl = (g[k].astype(np.float64) for k in ("r", "v", "d", "tl"))
    f = 1.0 - tl if filt else np.ones_like(tl)
    vn = np.concatenate([v[1:], lv[None]], 0)
    abar = (np.abs(r) + np.abs((1 - d) * gam * vn) + np.abs(v)) * f
    c = (1 - d) * gam * tau * f
    return adv[..., 0], ret[..., 0], _scan_bound(abar, c, v, adv[..., 0], T, np.zeros(N))


def discount_ref(g, filt, use_lt):
    """(adv, ret, bound) of trl_discount_reward_f32: a = r + tl v, c = nd gamma (1 - tl), y_T = last_value."""
    T, N = g["T"], g["N"]
    gam = F32(g["gamma"])
    lv = g["lv"].astype(np.float64) * (1.0 - g["lt"] if use_lt else 1.0)
    sh = lambda x: np.asarray(x, np.float64)[..., None]
    adv, ret = replay.discounted_return(sh(g["r"]), sh(g["v"]), sh(g["d"]), sh(g["tl"]), lv[:, None], gam, bool(filt))
    r, v, d, tl = (g[k].astype(np.float64) for k in ("r", "v", "d", "tl"))
    tlf = tl if filt else np.zeros_like(tl)
    abar = np.abs(r) + np.abs(tlf * v)
    c = (1 - d) * gam * (1 - tlf)
    return adv[..., 0], ret[..., 0], _scan_bound(abar, c, v, ret[..., 0], T, np.abs(lv))


def scan_f32(g, mode, filt, use_lt):
    """The recurrence step by step in float32 -> (adv, ret): what any float32 evaluation gives, held to the bounds."""
    T, N = g["T"], g["N"]
    f32 = np.float32
    gam, tau = f32(g["gamma"]), f32(g["tau"])
    lv = (g["lv"] * (f32(1) - g["lt"] if use_lt else f32(1))).astype(f32)
    y = np.zeros(N, f32) if mode == "gae" else lv.copy()
    adv, ret = np.zeros((T, N), f32), np.zeros((T, N), f32)
    for t in range(T - 1, -1, -1):
        nd = f32(1) - g["d"][t]
        tl = g["tl"][t] if filt else np.zeros(N, f32)
        if mode == "gae":
            vn = g["v"][t + 1] if t + 1 < T else lv
            a = ((g["r"][t] + nd * gam * vn - g["v"][t]) * (f32(1) - tl)).astype(f32)
            c = (nd * gam * tau * (f32(1) - tl)).astype(f32)
        else:
            a = (g["r"][t] + tl * g["v"][t]).astype(f32)
            c = (nd * gam * (f32(1) - tl)).astype(f32)
        y = (a + c * y).astype(f32)
        if mode == "gae":
            adv[t], ret[t] = y, y + g["v"][t]
        else:
            ret[t], adv[t] = y, y - g["v"][t]
    return adv, ret


def scan_ratios(g, mode, filt, use_lt, adv, ret):
    wa, wr, b = (gae_ref if mode == "gae" else discount_ref)(g, filt, use_lt)
    return _ratio(adv, wa, b + 1e-300), _ratio(ret, wr, b + 1e-300)


def grid_case(T=8, N=9):
    """Everything on a grid of 1/8, gamma = tau = 1, T <= 8: every float32 sum is exact, so float32 == float64."""
    rs = np.random.RandomState(5)
    k = lambda *s: (rs.randint(-16, 17, s) / 8.0).astype(np.float32)
    d = (rs.rand(T, N) < 0.2)
    return dict(T=T, N=N, r=k(T, N), v=k(T, N), d=d.astype(np.float32), tl=(d & (rs.rand(T, N) < 0.5)).astype(np.float32),
                lv=k(N), lt=(rs.rand(N) < 0.3).astype(np.float32), gamma=1.0, tau=1.0, planted={})
