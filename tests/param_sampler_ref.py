"""A NumPy statement of the vehicle-parameter draw (include/f110.h f110_param_dist): every env owns
np.random.Generator(PCG64(SeedSequence(seed, spawn_key=(env_base + e,)))); a draw walks the 18 parameters in PARAM_KEYS order,
and within a drawn one takes the env's single value (scope 'env') or one per agent in agent order (scope 'agent'):
Generator.uniform(a, b), or np.clip(Generator.normal(loc, scale), lo, hi); relative entries store nominal * value.  The calls
are NumPy's own, so everything is bitwise comparable with the device."""
import numpy as np

PARAM_KEYS = ['mu', 'C_Sf', 'C_Sr', 'lf', 'lr', 'h', 'm', 'I', 's_min', 's_max', 'sv_min', 'sv_max', 'v_switch', 'a_max', 'v_min',
              'v_max', 'width', 'length']


def generator_of_words(words):
    """the Generator whose PCG64 stands at the stream words {state.hi, state.lo, inc.hi, inc.lo}"""
    w = [int(v) for v in words]
    bg = np.random.PCG64(0)
    st = bg.state
    st["state"] = {"state": (w[0] << 64) | w[1], "inc": (w[2] << 64) | w[3]}
    st["has_uint32"], st["uinteger"] = 0, 0
    bg.state = st
    return np.random.Generator(bg)


def words_of_generator(gen):
    s = gen.bit_generator.state["state"]
    m = (1 << 64) - 1
    return np.array([s["state"] >> 64, s["state"] & m, s["inc"] >> 64, s["inc"] & m], dtype=np.uint64)


class ParamModel(object):
    """dists: {name: ('uniform', a, b, scope, relative) | ('normal', loc, scale, lo, hi, scope, relative)}; nominal [A][18];
    the generators from a seed (env e: spawn_key (env_base + e,)) or from stream words [E][4]"""

    def __init__(self, dists, nominal, num_envs, seed=None, env_base=0, words=None):
        self.dists = dict(dists)
        self.nominal = np.array(nominal, dtype=np.float64)
        self.E, self.A = int(num_envs), int(self.nominal.shape[0])
        if words is not None:
            self.gens = [generator_of_words(w) for w in words]
        else:
            self.gens = [np.random.Generator(np.random.PCG64(np.random.SeedSequence(seed, spawn_key=(int(env_base) + e,))))
                         for e in range(self.E)]
        self.rows = np.tile(self.nominal, (self.E, 1))   # [E * A][18]: armed, not yet drawn
        self.values = np.zeros(self.E, dtype=np.int64)   # values each env's stream has handed out

    def _value(self, e, d):
        self.values[e] += 1
        g = self.gens[e]
        if d[0] == "uniform":
            return g.uniform(d[1], d[2])
        return float(np.clip(g.normal(d[1], d[2]), d[3], d[4]))

    def draw(self, e):
        """one draw for env e; returns its rows [A][18] (also stored)"""
        A = self.A
        for p, name in enumerate(PARAM_KEYS):
            d = self.dists.get(name)
            if d is None:
                continue
            scope, relative = d[-2], d[-1]
            v = self._value(e, d) if scope == "env" else None
            for a in range(A):
                if scope != "env":
                    v = self._value(e, d)
                self.rows[e * A + a, p] = self.nominal[a, p] * v if relative else v
        return self.rows[e * A:(e + 1) * A]

    def draw_mask(self, mask):
        for e in np.flatnonzero(np.asarray(mask)):
            self.draw(int(e))
        return self.rows

    def words(self):
        return np.stack([words_of_generator(g) for g in self.gens])


def sampler_of(dists, seed):
    """the f1tenth_gym_amd.ParamSampler with the model's entries"""
    from f1tenth_gym_amd.param_sampler import ParamSampler, normal, uniform
    kw = {}
    for name, d in dists.items():
        kw[name] = uniform(d[1], d[2], scope=d[3], relative=d[4]) if d[0] == "uniform" else normal(d[1], d[2], d[3], d[4], scope=d[5], relative=d[6])
    return ParamSampler(seed, **kw)
