"""A CPU replay of sample_single_light's pick on the oracle's own vertices (no GPU; shared by tools/light_pick_replay.py and the tests).  The oracle has no
strategy 49, 113 or 177, so a sample is put together from what it has: kyo_trace_li gives the vertices of the both_mis path of (pixel, sample), kyo_li under
KY_DIRECT_IDLE and the same seed gives what that path adds without direct light (the path does not depend on the strategy), and kyo_kat_nee(48, light) gives each
light's two both_mis halves at a vertex for fresh numbers.  With nee[v, l] = luminance(beta_v x 0.5 x (the two halves of light l)):
  a sample under "one light l over p_l, l ~ p"  is   idle + sum_v nee[v, l_v] / p[v, l_v];
  given the path and the numbers its mean is          E = idle + sum_v sum_l nee[v, l]            (a both_mis sample), and its variance over the picks
                                                      P = sum_v (sum_l nee[v, l]^2 / p[v, l] - (sum_l nee[v, l])^2)   (picks are independent);
so a pixel's variance under a rule is var_s(E) + mean_s(P): the first part is every rule's, the second is what the pick adds."""
import numpy as np

import light_pick_restatement as R
from single_light_scenes import luminance

SHARES = (0.125, 0.25, 0.5)
RULES = ("uniform", "power", "spatial")


class Replay:
    """The vertices of `spp` samples of each pixel, every light's term at each, and the two rules' shares w / W (uniform where W is 0)"""

    def __init__(self, A, api, O, scene, W, H, pixels, spp, seed=1234, numbers_seed=20251020):
        self.A, self.n_pixels, self.spp = A, len(pixels), spp
        nl = self.nl = R.scene_view(api, scene).light_count
        p48 = api.make_params(W, H, spp, seed=seed, direct_sample=A.DIRECT_BOTH_MIS)
        idle = api.make_params(W, H, spp, seed=seed, direct_sample=A.DIRECT_IDLE)
        self.idle = np.stack([luminance(O.li(scene, idle, x, y, 0, spp)) for (x, y) in pixels])          # [pixels, spp]
        rows, pix, smp, first = [], [], [], np.zeros(len(pixels), np.int64)
        for i, (x, y) in enumerate(pixels):
            for s in range(spp):
                t = O.trace_li(scene, p48, x, y, s)
                if s == 0 and len(t):
                    first[i] = int(t[0, 1])
                t = t[(t[:, 2] == 0) | (t[:, 2] == 3)]                                                    # mirror and glass vertices take no estimate
                rows.append(t)
                pix.append(np.full(len(t), i))
                smp.append(np.full(len(t), s))
        t = np.concatenate(rows)
        self.pix, self.smp, self.first_surface = np.concatenate(pix), np.concatenate(smp), first
        rng = np.random.default_rng(numbers_seed)
        v = np.zeros((len(t), 16), np.float32)
        v[:, 0:9] = t[:, 3:12]                                                                            # position, normal, wo
        v[:, 9] = t[:, 1]
        v[:, 10] = np.where(t[:, 2] == 3, 0.0, R.BELOW_ONE)                                               # the lobe number that gives the traced lobe (2663)
        v[:, 11:15] = rng.uniform(0, 1, (len(t), 4))
        self.vertices = v
        beta = t[:, 12:15].astype(np.float64)
        nee = np.zeros((len(t), nl))
        for l in range(nl):
            h = O.kat_nee(scene, A.DIRECT_BOTH_MIS, l, v[:, :15]).astype(np.float64)
            nee[:, l] = luminance(beta * 0.5 * (h[:, 0:3] + h[:, 3:6]))
        self.dropped = int((~np.isfinite(nee)).any(axis=1).sum())                                          # (the reference's own inf x 0 at grazing hits)
        nee[~np.isfinite(nee).all(axis=1)] = 0.0
        self.nee = nee
        power = R.host_tables(A, api, scene)[2][:nl].astype(np.float64)
        self.share = {"uniform": np.full((len(t), nl), 1.0 / nl),
                      "power": np.broadcast_to(np.clip((power - R.SHARE / nl) / (1 - R.SHARE), 0, 1), (len(t), nl))}
        w = R.spatial_weights(A, api, scene, v).astype(np.float64)
        Wsum = w.sum(axis=1, keepdims=True)
        self.share["spatial"] = np.where(Wsum > 0, w / np.where(Wsum > 0, Wsum, 1), 1.0 / nl)

    def p(self, rule, a):
        return self.share[rule] if rule == "uniform" else a / self.nl + (1 - a) * self.share[rule]

    def _per_sample(self, per_vertex):
        out = np.zeros((self.n_pixels, self.spp))
        np.add.at(out, (self.pix, self.smp), per_vertex)
        return out

    def base(self):
        """E per sample [pixels, spp]: idle + every light's term at every vertex"""
        return self.idle + self._per_sample(self.nee.sum(axis=1))

    def pick_variance(self, rule, a=R.SHARE):
        """-> (per vertex, per pixel): what the pick adds, sum_l nee^2 / p - (sum_l nee)^2, and its mean over the samples of the sum over a sample's vertices"""
        pv = (self.nee ** 2 / self.p(rule, a)).sum(axis=1) - self.nee.sum(axis=1) ** 2
        return pv, self._per_sample(pv).mean(axis=1)

    def pixel_variance(self, rule, a=R.SHARE):
        return self.base().var(axis=1, ddof=1) + self.pick_variance(rule, a)[1]

    def ratio(self, rule, a=R.SHARE, pixels=None):
        """the summed per-pixel variance of a rule over the uniform pick's"""
        m = slice(None) if pixels is None else pixels
        return float(self.pixel_variance(rule, a)[m].sum() / self.pixel_variance("uniform")[m].sum())

    def draw(self, rule, a, rng, forget_p=False):
        """One sample per (pixel, sample) under the rule: idle + sum_v nee[v, l_v] / p[v, l_v], l_v ~ p; forget_p: times n instead (the likely bug)"""
        p = self.p(rule, a)
        cum = np.cumsum(p, axis=1)
        l = np.minimum((rng.uniform(0, 1, len(p))[:, None] >= cum).sum(axis=1), self.nl - 1)
        k = np.arange(len(p))
        x = self.nee[k, l] * (self.nl if forget_p else 1.0 / p[k, l])
        return self.idle + self._per_sample(x)
