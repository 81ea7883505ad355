"""Times of the exact t-SNE on one MI355X (profiles/tsne.md): the affinity stage (distances, perplexity search, joint) and the descent, per shape.
    python tools/tsne_probe.py                     the two shapes of profiles/tsne.md, 5 timed fits each after a warm-up
    python tools/tsne_probe.py --shape 2000 10 30  one shape of them
    python tools/tsne_probe.py --once 2000 10 30   one fit and nothing else: the run to put under rocprofv3 --kernel-trace --stats
    python tools/tsne_probe.py --sklearn           sklearn's TSNE on the host for the N = 2000 case (method="exact", then the default Barnes-Hut), if it imports
A host clock (time.perf_counter) between two torch.cuda.synchronize(); the fit synchronises the stream itself once per 50 iterations."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def blobs(N, d, seed=0):
    rng = np.random.RandomState(seed)
    centres = 4.0 * rng.standard_normal((10, d))
    return (centres[np.arange(N) % 10] + rng.standard_normal((N, d))).astype(np.float32)


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def one_fit(Zd, perplexity, Y0):
    from causal_vae_amd import ops
    (P, *_), t_aff = clock(lambda: ops.tsne_affinities_f64(ops.tsne_sqdist_f64(Zd), perplexity))
    fit, t_fit = clock(lambda: ops.tsne_fit_f64(P, Y0))
    return fit, t_aff, t_fit


def shape(N, d, perplexity, repeats):
    Zd = torch.as_tensor(blobs(N, d)).cuda()
    Y0 = torch.as_tensor(1e-4 * np.random.RandomState(42).standard_normal((N, 2)).astype(np.float32)).cuda().double()
    one_fit(Zd, perplexity, Y0)
    runs = [one_fit(Zd, perplexity, Y0) for _ in range(repeats)]
    aff, fit = sorted(r[1] for r in runs), sorted(r[2] for r in runs)
    f = runs[0][0]
    its = f.n_iter + 1
    med = fit[len(fit) // 2]
    print(f"TSNE N={N} d={d} perplexity={perplexity}: affinity stage {aff[len(aff) // 2]:.2f} ms ({aff[0]:.2f} - {aff[-1]:.2f}); descent {med:.1f} ms "
          f"({fit[0]:.1f} - {fit[-1]:.1f}) for {its} iterations and {f.checks} host reads: {med / its * 1e3:.1f} us per iteration; KL {f.kl:.5g}; "
          f"P is {N * N * 8 / 2 ** 20:.1f} MiB", flush=True)


def main():
    if "--sklearn" in sys.argv:
        try:
            from sklearn.manifold import TSNE
        except ImportError as e:
            print(f"sklearn does not import here: {e}")
            return
        Z = blobs(2000, 10)
        for kw in (dict(method="barnes_hut"), dict(method="exact")):
            t0 = time.perf_counter()
            m = TSNE(perplexity=30, init="random", random_state=42, verbose=2 if kw["method"] == "exact" else 0, **kw).fit(Z)
            print(f"sklearn TSNE {kw['method']} N=2000 d=10 on the host ({os.cpu_count()} CPUs seen): {time.perf_counter() - t0:.1f} s, KL {m.kl_divergence_:.5g}, "
                  f"n_iter_ {m.n_iter_}", flush=True)
        return
    if "--once" in sys.argv:
        N, d, perplexity = (int(v) for v in sys.argv[sys.argv.index("--once") + 1:][:3])
        Zd = torch.as_tensor(blobs(N, d)).cuda()
        Y0 = torch.as_tensor(1e-4 * np.random.RandomState(42).standard_normal((N, 2)).astype(np.float32)).cuda().double()
        fit, t_aff, t_fit = one_fit(Zd, float(perplexity), Y0)
        print(f"TSNE once N={N}: affinity stage {t_aff:.2f} ms, descent {t_fit:.1f} ms, {fit.n_iter + 1} iterations")
        return
    if "--shape" in sys.argv:          # one shape: for A/B runs of two builds (CVAE_HIP_LIB), a process each, alternating
        N, d, perplexity = (int(v) for v in sys.argv[sys.argv.index("--shape") + 1:][:3])
        shape(N, d, float(perplexity), 5)
        return
    shape(2000, 10, 30.0, 5)
    shape(4096, 512, 30.0, 5)


if __name__ == "__main__":
    main()
