"""One forward of the layout encoder at the LDM layout-to-image configuration (``BERTEmbedder(512, 16, vocab_size=8192, max_seq_len=92)``, 92 tokens per
sample), eager and as a captured graph, same process, no profiler.  Informational: no threshold -- the encoder runs once per batch against 50 or more UNet
evaluations, and bench.py does not time it.

    python tools/layout_encoder_time.py [windows] [batch ...]      # on the GPU; default 5 windows, batches 2 8 32

Timed: `windows` windows of >= 0.3 s of back-to-back forwards between two device events, after a warm-up.  FLOPs per sample, counted from the shapes:
per layer 2 L D (3 I + I + 8 D) for the four linears (I = 512, the inner width of 8 heads x 64) plus 4 L^2 I for the two attention products."""
import statistics
import sys

import torch

sys.path.insert(0, ".")
sys.path.insert(0, "tests")

D, LAYERS, VOCAB, L, INNER, WINDOW_S = 512, 16, 8192, 92, 512, 0.3


def flops_per_sample():
    return LAYERS * (2.0 * L * D * (4 * INNER + 8 * D) + 4.0 * L * L * INNER)


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / n


def windows_of(fn, windows):
    timed(fn, 3)
    count = max(3, int(WINDOW_S / timed(fn, 5)) + 1)
    evals = [timed(fn, count) for _ in range(windows)]
    return count, evals, statistics.median(evals)


def main(windows, batches):
    import layout_encoder_cases as ec
    from lfm_amd import hip
    from lfm_amd.models import BERTEmbedder

    dev = torch.device("cuda:0")
    m = BERTEmbedder(D, LAYERS, vocab_size=VOCAB, max_seq_len=L, use_tokenizer=False)
    ec.load_seeded(m)
    m = m.to(dev).eval()
    print(f"sustained clock under matrix load (lfm_clock_probe): {hip.effective_clock_mhz(dev):.0f} MHz")
    print(f"BERTEmbedder({D}, {LAYERS}, vocab_size={VOCAB}, max_seq_len={L}): {sum(p.numel() for p in m.parameters()) / 1e6:.1f} M parameters, "
          f"{flops_per_sample() / 1e9:.3f} GFLOP per sample of {L} tokens, {7 * LAYERS + 2} kernel launches per forward")
    for N in batches:
        tok = torch.randint(0, VOCAB, (N, L), generator=torch.Generator().manual_seed(N)).to(dev)
        eager = lambda: m(tok)  # noqa: E731
        count, evals, med = windows_of(eager, windows)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            m(tok)
        gcount, gevals, gmed = windows_of(graph.replay, windows)
        print(f"batch {N:3d} ({N * L} rows): eager {count} per window; ms " + " ".join(f"{v * 1e3:.3f}" for v in evals) +
              f"; median {med * 1e3:.3f} ms, spread {(max(evals) - min(evals)) / med * 100:.1f} %  |  captured graph {gcount} per window; ms " +
              " ".join(f"{v * 1e3:.3f}" for v in gevals) + f"; median {gmed * 1e3:.3f} ms, spread {(max(gevals) - min(gevals)) / gmed * 100:.1f} %; "
              f"{flops_per_sample() * N / gmed / 1e12:.2f} TFLOP/s")
        del graph


if __name__ == "__main__":
    a = [int(v) for v in sys.argv[1:]]
    main(a[0] if a else 5, a[1:] or [2, 8, 32])
