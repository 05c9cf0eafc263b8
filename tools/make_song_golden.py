"""Generate tests/golden/{song_tiny,song_wide,edm_cfg_grid}.pt by running the UNMODIFIED reference models/EDM.py and sampler/karras_sample.py on the CPU.

    python -m tools.make_song_golden            # where the reference checkout exists (LFM_REFERENCE, as oracle/make_golden.py)

Writes data only: configurations, seeded inputs, the reference's outputs and its state-dict key / shape list.  The SongUNet weights are NOT stored (3 M and
13 M parameters): both sides regenerate them from (name, shape, seed) with oracle/edm_state.py, as tests/golden/edm_full.pt does, and the fixture keeps a
checksum.  That seeded state leaves no tensor at the reference's 0 / 1e-5 initialisation, so every path of the network matters (the default-initialised
reference outputs ~6e-6)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import song_cases as sc  # noqa: E402
from oracle.make_golden import OUT, _import_reference  # noqa: E402


def _emb_hook(m, store):
    """Record the reference's mapping-network output emb = silu(map_layer1(.)) of the next evaluation."""
    def hook(mod, inp, outp):
        store.append(torch.nn.functional.silu(outp.detach()).clone())
    return m.map_layer1.register_forward_hook(hook)


def golden_song(ref_edm, cfg, batch, with_solve, load=sc.load_seeded):
    m = ref_edm.SongUNet(**cfg).eval()
    rec = {"cfg": cfg, "state_seed": sc.STATE_SEED, "state_checksum": load(m), "params": sum(p.numel() for p in m.parameters()),
           "keys": [(k, tuple(v.shape)) for k, v in m.state_dict().items()]}
    g = torch.Generator().manual_seed(31 + batch)
    R, C = cfg["img_resolution"], cfg["in_channels"]
    x = torch.randn(batch, C, R, R, generator=g)
    tN = torch.tensor([0.9, 0.5, 0.3, 0.05])[:batch]
    rec["x"], rec["tN"] = x, tN
    y = torch.tensor([1, 4, 0, 2])[:batch] if cfg["label_dim"] else None
    with torch.no_grad():
        if y is not None:
            rec["y"] = y
            embs = []
            h = _emb_hook(m, embs)
            rec["v_t0d"] = m(torch.tensor(0.6), x, y)
            rec["v_tN"] = m(tN, x, y)
            h.remove()
            rec["emb_t0d"], rec["emb_tN"] = embs
            # "without labels" is the label_dim = 0 model on the same weights: the reference's forward cannot take y=None when it has a map_label
            m0 = ref_edm.SongUNet(**dict(cfg, label_dim=0)).eval()
            m0.load_state_dict({k: v for k, v in m.state_dict().items() if not k.startswith("map_label.")}, strict=True)
            rec["v_nolabel"] = m0(torch.tensor(0.6), x)
        else:
            rec["v_t0d"] = m(torch.tensor(0.6), x)
            rec["v_tN"] = m(tN, x)
        if with_solve:
            from lfm_amd.solvers import torchdiffeq_euler_grid

            ts, dts = torchdiffeq_euler_grid(0.1)  # odeint(..., t=[1, 0], method="euler", options={"step_size": 0.1}): x += dt * v(t, x)
            xs = x.clone()
            for k in range(dts.numel()):
                xs = xs + dts[k] * (m(ts[k], xs, y) if y is not None else m(ts[k], xs))
            rec["x_euler10"] = xs
    print(cfg["model_channels"], "params", rec["params"], "tensors", len(rec["keys"]), "|v|", float(rec["v_t0d"].abs().mean()), flush=True)
    return rec


def golden_edm_cfg_grid(ref_edm, ref_karras):
    """Guided DhariwalUNet (edm_tiny.pt's configuration and weights) on the fixed grids, by the reference's forward_with_cfg and its own samplers."""
    from lfm_amd.solvers import torchdiffeq_euler_grid

    tiny = torch.load(os.path.join(OUT, "edm_tiny.pt"), map_location="cpu", weights_only=False)
    m = ref_edm.DhariwalUNet(**tiny["cfg"]).eval()
    m.load_state_dict({k: (v.float() if v.is_floating_point() else v) for k, v in tiny["state_dict"].items()}, strict=True)
    g = torch.Generator().manual_seed(57)
    half = torch.randn(2, 4, 16, 16, generator=g)
    x = torch.cat([half, half], 0)  # the guidance doubling of test_flow_latent.py:163-183: [x, x], labels [y, zeros]
    y = torch.tensor([3, 1, 0, 0])
    rec = {"x": x, "y": y, "cfg_scale": 1.7, "steps": 6}
    kw = dict(y=y, cfg_scale=1.7)
    with torch.no_grad():
        ts, dts = torchdiffeq_euler_grid(0.1)
        xs = x.clone()
        for k in range(dts.numel()):
            xs = xs + dts[k] * m.forward_with_cfg(ts[k], xs, **kw)
        rec["x_euler10"] = xs
        for sampler in ("euler", "heun"):  # the arguments of sample_from_model_with_fixed_step_solver (test_flow_latent.py:79-97)
            rec["x_karras_" + sampler] = ref_karras.karras_sample(m, x, steps=6, model_kwargs=kw, device="cpu", clip_denoised=False, sigma_min=1e-5,
                                                                  sigma_max=1.0, s_tmin=0.0, s_tmax=1.0, s_churn=0.0, sampler=sampler)
    return rec


def main():
    _, ref_karras, _ = _import_reference()
    import models.EDM as ref_edm

    torch.save(golden_song(ref_edm, sc.TINY_CFG, 4, True), os.path.join(OUT, "song_tiny.pt"))
    torch.save(golden_song(ref_edm, sc.WIDE_CFG, 2, False), os.path.join(OUT, "song_wide.pt"))
    torch.save(golden_edm_cfg_grid(ref_edm, ref_karras), os.path.join(OUT, "edm_cfg_grid.pt"))


if __name__ == "__main__":
    main()
