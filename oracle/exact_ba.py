"""One synchronous_iteration of the reference's BA graph from a complete state, at two precisions (TEST INFRASTRUCTURE ONLY --
imported by tests/, never by gbp_amd/).

Dense information form, exactly as joeaortiz/gbp does it, vectorised over factors:

  robustify               gbp/gbp.py:296-332        relinearisation test     gbp/gbp.py:64-80
  compute_factor          gbp/gbp.py:267-294        damping switch           gbp/gbp.py:46-54
  compute_messages        gbp/gbp.py:334-373        update_belief            gbp/gbp.py:176-198
  meas_fn / jac_fn        gbp/factors/reprojection.py:12-44, utils/derivatives.py:36-50, utils/lie_algebra.py:32-42

One code path, two kinds of number:
  * dps=None: float64, the reference's formulas with np.linalg.inv where the reference has it -- the YARDSTICK, what dense float64
    maths of the reference's kind achieves from the same state.  Not the reference's bits: the products are batched over factors
    (numpy may sum them in another order), and on fixture G4 this path is 4.5e-11 from the reference's it2 where the exact run is
    2.8e-11 (tests/test_exact_ba.py);
  * dps=k:    mpmath at k significant digits (object arrays, unpivoted Gauss-Jordan: every matrix inverted here is SPD) -- "exact".

The state is a dict of float64 arrays (reference factor order; cameras first, then landmarks, as in BAFactorGraph):
  K (4,) fx fy cx cy; cam_prior_eta (C,6), cam_prior_lam (C,6,6), lmk_prior_eta (L,3), lmk_prior_lam (L,3,3);
  msg_cam_eta (F,6), msg_cam_lam (F,6,6), msg_lmk_eta (F,3), msg_lmk_lam (F,3,3): the factors' current messages;
  linpoint (F,9), z (F,2), cam (F,), lmk (F,), adaptive_var (F,), iters_since_relin (F,), eta_damping (F,).
The beliefs the factors read are prior + sum of messages (update_belief), formed here.  sweep() returns the next state plus
cam_eta / cam_lam / lmk_eta / lmk_lam / cam_mu / lmk_mu (the new beliefs), relin and robust_flag (the decisions taken).
"""
from __future__ import annotations

import numpy as np

TIE = 1e-9        # relative distance to a decision threshold below which the caller's forced decision is not checked


class _F64:
    """float64 arithmetic, the reference's routines."""
    exact = False

    def conv(self, a):
        return np.array(a, dtype=np.float64)

    def inv(self, A):
        return np.linalg.inv(A)

    sqrt, sin, cos = staticmethod(np.sqrt), staticmethod(np.sin), staticmethod(np.cos)

    def tofloat(self, a):
        return np.asarray(a, dtype=np.float64)


class _MP:
    """mpmath arithmetic at `dps` digits on object arrays."""
    exact = True

    def __init__(self, mp):
        self.mp = mp
        self._conv = np.vectorize(lambda x: mp.mpf(float(x)) if not isinstance(x, type(mp.mpf(0))) else x, otypes=[object])
        self.sqrt = np.vectorize(mp.sqrt, otypes=[object])
        self.sin = np.vectorize(mp.sin, otypes=[object])
        self.cos = np.vectorize(mp.cos, otypes=[object])
        self._tof = np.vectorize(float, otypes=[np.float64])

    def conv(self, a):
        a = np.asarray(a)
        return self._conv(a) if a.size else a.astype(object)

    def inv(self, A):
        """Batched unpivoted Gauss-Jordan, (..., n, n)."""
        A = A.copy()
        n = A.shape[-1]
        X = np.zeros(A.shape, dtype=object)
        X[...] = self.mp.mpf(0)
        for i in range(n):
            X[..., i, i] = self.mp.mpf(1)
        for k in range(n):
            p = A[..., k, k][..., None].copy()
            A[..., k, :] = A[..., k, :] / p
            X[..., k, :] = X[..., k, :] / p
            for i in range(n):
                if i != k:
                    c = A[..., i, k][..., None].copy()
                    A[..., i, :] = A[..., i, :] - c * A[..., k, :]
                    X[..., i, :] = X[..., i, :] - c * X[..., k, :]
        return X

    def tofloat(self, a):
        a = np.asarray(a)
        return self._tof(a) if a.size else a.astype(np.float64)


def _hat(ar, v):
    z = ar.conv(np.zeros(v.shape[:-1]))
    return np.stack([np.stack([z, -v[..., 2], v[..., 1]], -1), np.stack([v[..., 2], z, -v[..., 0]], -1),
                     np.stack([-v[..., 1], v[..., 0], z], -1)], -2)


def _so3exp(ar, w):
    """lie_algebra.so3exp, batched: I below 3 eps."""
    n = w.shape[0]
    th = ar.sqrt(np.sum(w * w, axis=1))
    small = np.array([bool(t < 3 * np.finfo(float).eps) for t in th], dtype=bool)
    ths = np.where(small, ar.conv(np.ones(n)), th)
    wh = _hat(ar, w)
    eye = ar.conv(np.broadcast_to(np.eye(3), (n, 3, 3)))
    R = eye + (ar.sin(ths) / ths)[:, None, None] * wh + ((1 - ar.cos(ths)) / ths ** 2)[:, None, None] * (wh @ wh)
    R[small] = eye[small]
    return R


def meas_jac(ar, x, K4):
    """reprojection.meas_fn and jac_fn at the rows of x (F,9): h (F,2), J (F,2,9)."""
    n = x.shape[0]
    fx, fy, cx, cy = (K4[i] for i in range(4))
    zero, one = ar.conv(0.0), ar.conv(1.0)
    K = np.array([[fx, zero, cx], [zero, fy, cy], [zero, zero, one]], dtype=K4.dtype)
    t, w, y = x[:, 0:3], x[:, 3:6], x[:, 6:9]
    R = _so3exp(ar, w)
    p = np.einsum('ij,fj->fi', K, np.einsum('fij,fj->fi', R, y) + t) if not ar.exact else \
        (K[None] @ ((R @ y[..., None])[..., 0] + t)[..., None])[..., 0]
    h = p[:, :2] / p[:, 2:3]
    Jp = ar.conv(np.zeros((n, 2, 3)))                              # derivatives.proj_derivative
    Jp[:, 0, 0] = 1 / p[:, 2]
    Jp[:, 1, 1] = 1 / p[:, 2]
    Jp[:, :, 2] = -p[:, :2] / (p[:, 2:3] ** 2)
    JpK = Jp @ K[None]
    eye = ar.conv(np.broadcast_to(np.eye(3), (n, 3, 3)))
    dR = -((R @ _hat(ar, y)) @ (np.einsum('fi,fj->fij', w, w) + (np.swapaxes(R, 1, 2) - eye) @ _hat(ar, w))
           / np.sum(w * w, axis=1)[:, None, None])                 # derivatives.dR_wx_dw
    J = np.concatenate([JpK, JpK @ dR, JpK @ R], axis=2)
    return h, J


def _near(a, b):
    return abs(float(a) - float(b)) <= TIE * max(abs(float(b)), 1e-300)


def sweep(state, *, sigma2, loss=None, nstds=3.0, beta=0.01, num_undamped_iters=6, min_linear_iters=8, eta_damping=0.4,
          dps=None, relin=None, robust=None):
    """One synchronous_iteration(robustify=True, local_relin=True).  relin / robust (bool (F,)): the caller's decisions, taken instead
    of this sweep's own; the exact run asserts it would decide the same except within TIE of a threshold."""
    if dps is None:
        return _sweep(_F64(), state, sigma2, loss, nstds, beta, num_undamped_iters, min_linear_iters, eta_damping, relin, robust)
    import mpmath
    ctx = mpmath.MPContext()
    ctx.dps = int(dps)
    return _sweep(_MP(ctx), state, sigma2, loss, nstds, beta, num_undamped_iters, min_linear_iters, eta_damping, relin, robust)


def beliefs(ar, st):
    """update_belief (gbp.py:176-198): prior + messages in ascending factor order; Sigma = inv(Lambda), mu = Sigma eta."""
    cam, lmk = np.asarray(st['cam']), np.asarray(st['lmk'])
    ce, cl = ar.conv(st['cam_prior_eta']), ar.conv(st['cam_prior_lam'])
    le, ll = ar.conv(st['lmk_prior_eta']), ar.conv(st['lmk_prior_lam'])
    np.add.at(ce, cam, st['msg_cam_eta'])
    np.add.at(cl, cam, st['msg_cam_lam'])
    np.add.at(le, lmk, st['msg_lmk_eta'])
    np.add.at(ll, lmk, st['msg_lmk_lam'])
    cS, lS = ar.inv(cl), ar.inv(ll)
    return ce, cl, le, ll, (cS @ ce[..., None])[..., 0], (lS @ le[..., None])[..., 0]


def _sweep(ar, st, sigma2, loss, nstds, beta, num_undamped, min_linear, damping, relin_in, robust_in):
    F = st['linpoint'].shape[0]
    cam, lmk = np.asarray(st['cam'], dtype=np.int64), np.asarray(st['lmk'], dtype=np.int64)
    K4 = ar.conv(st['K'])
    x0, z = ar.conv(st['linpoint']), ar.conv(st['z'])
    m = {k: ar.conv(st[k]) for k in ('msg_cam_eta', 'msg_cam_lam', 'msg_lmk_eta', 'msg_lmk_lam')}
    s0 = dict(st, **m)
    ce, cl, le, ll, cmu, lmu = beliefs(ar, s0)
    s2 = ar.conv(sigma2)
    # robustify_loss (gbp.py:296-332): Mahalanobis distance of the residual at the linearisation point
    if loss is None:
        avar = ar.conv(np.full(F, float(sigma2)))
        rflag = np.zeros(F, bool)
    else:
        h0, _ = meas_jac(ar, x0, K4)
        r = z - h0
        md = ar.sqrt(r[:, 0] ** 2 + r[:, 1] ** 2) / ar.sqrt(s2)
        own = np.array([bool(v > nstds) for v in md], dtype=bool)
        rflag = own if robust_in is None else np.asarray(robust_in, dtype=bool)
        if ar.exact and robust_in is not None:
            bad = [f for f in range(F) if own[f] != rflag[f] and not _near(md[f], nstds)]
            assert not bad, f"robust flag forced against the exact decision at factors {bad[:8]}"
        mdr = np.where(rflag, md, ar.conv(np.full(F, 2.0 * nstds)))   # (the robust formulas only where they apply)
        if loss == 'huber':
            rob = s2 * mdr ** 2 / (2 * (nstds * mdr - 0.5 * nstds ** 2))
        else:
            rob = mdr ** 2
        avar = np.where(rflag, rob, ar.conv(np.full(F, float(sigma2))))
    # relinearise_factors (gbp.py:64-80)
    means = np.concatenate([cmu[cam], lmu[lmk]], axis=1)
    dist = ar.sqrt(np.sum((x0 - means) ** 2, axis=1))
    iters = np.asarray(st['iters_since_relin'], dtype=np.int64).copy()
    old_enough = iters >= min_linear
    own = np.array([bool(dd > beta) for dd in dist], dtype=bool) & old_enough
    relin = own if relin_in is None else np.asarray(relin_in, dtype=bool)
    if ar.exact and relin_in is not None:
        bad = [f for f in range(F) if own[f] != relin[f] and not (old_enough[f] and _near(dist[f], beta))]
        assert not bad, f"relinearisation forced against the exact decision at factors {bad[:8]}"
    x0 = np.where(relin[:, None], means, x0)
    iters = np.where(relin, 0, iters + 1)
    d = np.where(relin, 0.0, np.asarray(st['eta_damping'], dtype=np.float64))
    d = np.where(iters == num_undamped, float(damping), d)           # gbp.py:50-51
    # compute_factor (gbp.py:267-294) at the (new) linearisation point
    h, J = meas_jac(ar, x0, K4)
    Jt = np.swapaxes(J, 1, 2)
    lam_f = (Jt / avar[:, None, None]) @ J
    eta_f = ((Jt / avar[:, None, None]) @ ((J @ x0[..., None])[..., 0] + z - h)[..., None])[..., 0]
    # compute_messages (gbp.py:334-373): product with the other variable's cavity, then eliminate it
    dd = ar.conv(d)
    out = {}
    for v, (o, s, be, bl, me, ml, okey) in enumerate(((slice(0, 6), slice(6, 9), le[lmk], ll[lmk], m['msg_lmk_eta'], m['msg_lmk_lam'], 'cam'),
                                                      (slice(6, 9), slice(0, 6), ce[cam], cl[cam], m['msg_cam_eta'], m['msg_cam_lam'], 'lmk'))):
        eta, lam = eta_f.copy(), lam_f.copy()
        eta[:, s] = eta[:, s] + (be - me)
        lam[:, s, s] = lam[:, s, s] + (bl - ml)
        inv = ar.inv(lam[:, s, s])
        lono, lnoo = lam[:, o, s], lam[:, s, o]
        out[f'msg_{okey}_lam'] = lam[:, o, o] - (lono @ inv) @ lnoo
        new_eta = eta[:, o] - ((lono @ inv) @ eta[:, s][..., None])[..., 0]
        out[f'msg_{okey}_eta'] = (1 - dd)[:, None] * new_eta + dd[:, None] * m[f'msg_{okey}_eta']
    nxt = dict(st)
    nxt.update(out)
    ce, cl, le, ll, cmu, lmu = beliefs(ar, nxt)
    tf = ar.tofloat
    res = dict(st)
    res.update({k: tf(v) for k, v in out.items()})
    res.update(cam_eta=tf(ce), cam_lam=tf(cl), lmk_eta=tf(le), lmk_lam=tf(ll), cam_mu=tf(cmu), lmk_mu=tf(lmu),
               linpoint=tf(x0), adaptive_var=tf(avar), iters_since_relin=iters.astype(np.int32), eta_damping=d.astype(np.float64),
               relin=relin, robust_flag=rflag)
    if ar.exact:                                   # full-precision copies, for precision checks
        res['_exact'] = dict(cam_eta=ce, cam_lam=cl, lmk_eta=le, lmk_lam=ll, cam_mu=cmu, lmk_mu=lmu)
    return res


def state_from_engine(g, K, priors=None):
    """The complete state of an object with the BAEngine views (priors / messages / factors(dense=False) / relin_state)."""
    ce, cl, le, ll = g.priors() if priors is None else priors
    me, ml, ne, nl = g.messages()
    fa = g.factors(dense=False)
    rs = g.relin_state()
    return dict(K=np.asarray(K, dtype=np.float64).reshape(4), cam_prior_eta=ce, cam_prior_lam=cl, lmk_prior_eta=le, lmk_prior_lam=ll,
                msg_cam_eta=me, msg_cam_lam=ml, msg_lmk_eta=ne, msg_lmk_lam=nl, linpoint=fa['linpoint'], z=fa['z'],
                cam=fa['cam'].astype(np.int64), lmk=fa['lmk'].astype(np.int64), adaptive_var=rs['adaptive_var'],
                iters_since_relin=rs['iters_since_relin'].astype(np.int64), eta_damping=rs['eta_damping'],
                robust_flag=rs['robust_flag'].astype(bool))


def mahalanobis(mu, mu_ref, lam_ref):
    """max over variables of sqrt(d^T Lambda d), d = mu - mu_ref: a mean error in standard deviations of the reference belief."""
    dlt = np.asarray(mu, dtype=np.float64) - np.asarray(mu_ref, dtype=np.float64)
    q = np.einsum('vi,vij,vj->v', dlt, np.asarray(lam_ref, dtype=np.float64), dlt)
    return float(np.sqrt(np.maximum(q, 0.0)).max()) if q.size else 0.0
