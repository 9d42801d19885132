"""What the exact-arithmetic tests of the SE(3) / SE(2) factor models share (test_linear_se3_exact_cpu.py, test_linear_se3_exact_gpu.py):
fixture G31 (tests/golden/make_g31.py: the models from their definitions at 60 digits, rounded to double), its blocks, the bounds and
the measure of a gap.  Nothing here needs mpmath or a GPU."""
import numpy as np

from conftest import golden

EPS = 2.0 ** -52
# The bounds, from rounding alone.  h: phi is the Log of a product of two rotation matrices whose entries are each a few eps off, times
# a condition of about pi; u is a 3-term product sum of such entries.  eta_f, Lambda_f, energy, m2: products of two such quantities.
# They hold for EVERY block, pi - |phi| = 1e-8 included, on the host build and on the device alike.
# Observed, the worst block of each quantity.  Host build: h 2.3e-15 (twopi), eta 2.6e-15 (pastpi), lam 1.9e-15 (twopi), energy and m2
# 1.0e-15 (twopi); every pi-G block: h <= 7.6e-16, eta <= 1.6e-15.  SE(2): h 2.2e-16, eta 7.2e-16, lam 5.7e-16, energy and m2 5.2e-16.
# The twin: h 2.3e-15, eta 4.6e-15 (pi-1e-08), lam 2.5e-15, energy and m2 1.3e-15.  The MI355X: eta 1.9e-15 (twopi), lam 2.3e-15 (twopi),
# m2 1.5e-15 (pastpi), the block energies within 0.7 % of their bound; SE(2): eta 4.7e-15 (of which the read-out through joint_eta() is
# up to 21 eps), lam 4.4e-16, m2 8.7e-16.
# What the bounds caught.  With the skew-part Log and the (1 + cos) / sin coefficient the host build misses on the blocks pi - |phi| <=
# 1e-2: h 1.6e-14 (1e-2), 2.8e-13 (1e-3), 1.1e-12 (1e-4), 8.0e-11 (1e-6), 2.6e-8 (1e-8).  With b = J x0 + diag(s) z - h summed term by
# term the SE(2) routine misses at theta = 1e6: eta 4.7e-12.
H_TOL = 64 * EPS                 # 1.4e-14
F_TOL = 256 * EPS                # 5.7e-14
QUANTITIES = ('h', 'eta', 'lam', 'energy', 'm2')
TOLS = dict(h=H_TOL, eta=F_TOL, lam=F_TOL, energy=F_TOL, m2=F_TOL)


def fixture():
    return golden('G31_se3_exact')


def blocks(g):
    """[(name, indices)] of the SE(3) points by class, in the fixture's order."""
    cls = g['cls']
    return [(str(name), np.nonzero(cls == k)[0]) for k, name in enumerate(g['classes'])]


def exact(g, prefix=''):
    return tuple(g[prefix + k] for k in QUANTITIES)


def gaps(got, want, names=QUANTITIES):
    """Per point and quantity, as _close of test_linear_se3_cpu.py measures: max |got - want| relative to the larger of 1 and the point's
    largest exact entry.  {quantity: (n,)}; a value that is not finite is an infinite gap."""
    out = {}
    for name, a, b in zip(names, got, want):
        a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
        a, b = a.reshape(a.shape[0], -1), b.reshape(b.shape[0], -1)
        d = np.abs(a - b).max(1) / np.maximum(1.0, np.abs(b).max(1))
        out[name] = np.where(np.all(np.isfinite(a), 1), d, np.inf)
    return out


def report_and_check(what, gap, parts):
    """Print the worst gap per block and quantity, then assert every one of them against its bound."""
    bad = []
    for name, idx in parts:
        row = {q: float(gap[q][idx].max()) for q in gap}
        print(f'{what} {name:10s} ' + '  '.join(f'{q} {v:.2e}' for q, v in row.items()))
        bad += [f'{name}: {q} {v:.3e} > {TOLS[q]:.3e} at point {idx[gap[q][idx].argmax()]}' for q, v in row.items() if not v < TOLS[q]]
    assert not bad, f'{what}: ' + '; '.join(bad)
