#!/usr/bin/env python3
"""What the LM-fused CTC prefix beam search (``ocrvi_ctc_beam_lm``) costs beside ``ocrvi_ctc_beam`` on the same inputs.  Prints ONE JSON line.

  kernel   B = 256, T = 80, C = 232, W in 1, 4, 8, 16, 32, 64 (nbest = min(W, 4)) on the two row kinds of tools/ctc_beam_bench.py (the
           log-probabilities SVTRv2-base gives 256 synthetic crops with seeded weights: flat rows; text-like rows: peaked), with four
           tables: order 1 (unigrams only: no table probe after the start, so what remains is selection and barriers), order 4 with about
           1e4 entries (stays in an XCD's L2), order 4 with about 1e6 entries (32 MiB of slots: the Infinity Cache) and order 6 with about
           1e5.  Beside every width ``ocrvi_ctc_beam`` on the same rows in the same process, and once the f16x2 ``ocrvi_rec_forward`` of
           the same crops.  HIP events around every launch, warm, the median.
  engine   ``Engine.run`` on tools/engine_bench.py's 64 pages of 960 x 1280 with ``beam=None``, ``beam=8, nbest=4`` and ``beam=8,
           nbest=4, lm=...`` (an order-4 model trained on synthetic lines), each twice, alternating.

Every step runs in a child process of its own under a time limit; after a step that fails or runs out of time nothing more is started."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

WIDTHS = (1, 4, 8, 16, 32, 64)
STEP_LIMIT_S = {"kernel": 420, "engine": 540}


def random_lm(seed, order, entries, num_classes=232):
    """A CharLM with every unigram and about ``entries`` random longer grams, spread evenly over the levels 2..order."""
    import numpy as np
    from ocr_vi_invoice_amd import _lib
    from ocr_vi_invoice_amd.lm import CharLM
    rng = np.random.default_rng(seed)
    rows = [np.concatenate([np.arange(1, num_classes)[:, None], np.full((num_classes - 1, 5), -1)], 1)]
    lens = [np.ones(num_classes - 1, np.int64)]
    for k in range(2, order + 1):
        n = max(entries - (num_classes - 1), 0) // (order - 1)
        g = rng.integers(1, num_classes, (n, k))
        g[rng.random(n) < 0.1, 0] = 0                                    # a tenth start at the line start
        g = np.unique(g, axis=0)
        rows.append(np.concatenate([g, np.full((len(g), _lib.LM_MAX_ORDER - k), -1)], 1))
        lens.append(np.full(len(g), k))
    ids, lens = np.concatenate(rows).astype(np.int32), np.concatenate(lens).astype(np.int32)
    lp = (-6.0 * rng.random(len(ids))).astype(np.float32)
    bo = (-rng.random(len(ids))).astype(np.float32)
    return CharLM(ids, lens, lp, bo, order, num_classes, 0, -8.0)


def _median_ms(fn, iters):
    import torch
    for _ in range(3):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
    return {"ms_median": round(ms[len(ms) // 2], 4), "ms_min_max": [round(ms[0], 4), round(ms[-1], 4)], "launches": iters}


def step_kernel(args):
    import numpy as np
    import torch
    import ctcbeam_ref as BR
    from ocr_vi_invoice_amd import SVTRv2, synth, weights
    B, H, W_img = 256, 48, 320
    T, C = W_img // 4, 232
    rec = SVTRv2("base", state_dict=weights.make_rec_state_dict("base", seed=1234), dtype="f16x2")
    x = torch.from_numpy(synth.pad_crop_batch(synth.make_crops(7, B, height=H, max_width=W_img), H, W_img)).cuda()
    st = torch.cuda.current_stream().cuda_stream
    ws = rec._workspace(B, H, W_img)
    lp = torch.empty((T, B, C), dtype=torch.float32, device="cuda")
    am, ids, lens = (torch.empty((B, T), dtype=torch.int32, device="cuda"), torch.empty((B, T), dtype=torch.int32, device="cuda"),
                     torch.empty(B, dtype=torch.int32, device="cuda"))

    def forward():
        rec.enqueue_forward(x.data_ptr(), B, H, W_img, lp.data_ptr(), am.data_ptr(), ids.data_ptr(), lens.data_ptr(), ws.data_ptr(), ws.numel(), st)

    res = {"B": B, "T": T, "C": C, "rec_forward_f16x2_base_256x48x320": _median_ms(forward, args.iters)}
    tables = {"order1_unigrams": random_lm(1, 1, 0), "order4_1e4": random_lm(2, 4, 10_000), "order4_1e6": random_lm(3, 4, 1_000_000),
              "order6_1e5": random_lm(4, 6, 100_000)}
    res["tables"] = {k: {"entries": len(m), "slot_bytes": len(m.blob) - 48} for k, m in tables.items()}
    for m in tables.values():
        m.to("cuda:0")
    peaked = torch.from_numpy(np.ascontiguousarray(np.stack([BR.text_like(100 + b, T, C, 8.0) for b in range(B)], 1))).cuda()
    for name, rows in (("model_rows", lp.clone()), ("text_like_rows", peaked)):
        out = {}
        for W in WIDTHS:
            nbest = min(W, 4)
            bws = torch.empty(rec.beam_lm_workspace_bytes(T, B, W), dtype=torch.uint8, device="cuda")
            hid = torch.empty((B, nbest, T), dtype=torch.int32, device="cuda")
            hlen = torch.empty((B, nbest), dtype=torch.int32, device="cuda")
            hsc = [torch.empty((B, nbest), dtype=torch.float64, device="cuda") for _ in range(3)]

            def beam():
                rec.enqueue_beam(rows.data_ptr(), T, B, W, nbest, hid.data_ptr(), hlen.data_ptr(), hsc[0].data_ptr(), bws.data_ptr(), bws.numel(), st)

            row = {"ctc_beam": _median_ms(beam, args.iters)}
            for tname, m in tables.items():
                def beam_lm():
                    rec.enqueue_beam_lm(rows.data_ptr(), T, B, W, nbest, m, 0.5, 0.5, hid.data_ptr(), hlen.data_ptr(), *[s.data_ptr() for s in hsc],
                                        bws.data_ptr(), bws.numel(), st)

                row[tname] = _median_ms(beam_lm, args.iters)
            out[f"W{W}"] = row
        fwd = res["rec_forward_f16x2_base_256x48x320"]["ms_median"]
        out["beam_lm_order4_1e4_W8_over_rec_forward"] = round(out["W8"]["order4_1e4"]["ms_median"] / fwd, 4)
        res[name] = out
    return res


def step_engine(args):
    import engine_bench as EB
    import torch
    import ctclm_ref as LR
    from ocr_vi_invoice_amd import DBNetPP, SVTRv2, weights
    from ocr_vi_invoice_amd.lm import CharLM
    from ocr_vi_invoice_amd.pipeline import DBPostProcessor
    det = DBNetPP(pretrained=False, dtype="f16x2", state_dict=weights.make_det_state_dict(seed=1234))
    rec = SVTRv2("base", state_dict=weights.make_rec_state_dict("base", seed=1234), dtype="f16x2")
    pp = DBPostProcessor(thresh=0.3, box_thresh=0.5, max_candidates=1000, unclip_ratio=1.6)
    lm = CharLM.train(LR.synthetic_lines(7, 2000), rec.tokenizer, order=4)
    kw = dict(rec_size=(48, 320), det_chunk=16, rec_batch=256)
    ns = argparse.Namespace(lines=30, warmup=args.warmup, steps=args.steps)
    sizes = [(960, 1280)] * args.pages
    runs = {"lm_entries": len(lm)}
    sets = (("beam_none", {}), ("beam8_nbest4", dict(beam=8, nbest=4)), ("beam8_nbest4_lm", dict(beam=8, nbest=4, lm=lm, lm_weight=0.5, len_bonus=0.5)))
    for rnd in ("", "_again"):
        for name, extra in sets:
            r = EB.run_set(f"uniform 960x1280 {name}", dict(kw, **extra), sizes, 1280, ns, det, rec, pp)
            runs[name + rnd] = {k: r[k] for k in ("ms_per_run_median", "ms_per_run_min_max", "pages_per_s", "crops", "rec_batches", "host_ms_per_run")}
            torch.cuda.synchronize()
    base = runs["beam_none"]["ms_per_run_median"]
    runs["beam8_lm_over_none_percent"] = round(100.0 * (runs["beam8_nbest4_lm"]["ms_per_run_median"] / base - 1.0), 2)
    runs["beam8_lm_over_beam8_percent"] = round(100.0 * (runs["beam8_nbest4_lm"]["ms_per_run_median"] / runs["beam8_nbest4"]["ms_per_run_median"] - 1.0), 2)
    return runs


STEPS = {"kernel": step_kernel, "engine": step_engine}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS), help="run this step in this process (what the driver starts)")
    ap.add_argument("--steps-list", default="kernel,engine", help="the steps the driver runs, in order")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pages", type=int, default=64)
    args = ap.parse_args()
    if args.step:
        import torch
        assert torch.cuda.is_available(), "ctc_beam_lm_bench needs a GPU"
        torch.cuda.set_device(0)
        print(json.dumps(STEPS[args.step](args)), flush=True)
        return 0
    res = {"tool": "ctc_beam_lm_bench", "iters": args.iters, "steps": args.steps, "warmup": args.warmup, "pages": args.pages}
    rc = 0
    for name in args.steps_list.split(","):
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S[name]), sys.executable, os.path.abspath(__file__), "--step", name, "--iters",
               str(args.iters), "--steps", str(args.steps), "--warmup", str(args.warmup), "--pages", str(args.pages)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:                                           # a failed or timed-out step: nothing more is started
            res[name] = {"failed": p.returncode}
            rc = 1
            break
        res[name] = json.loads(p.stdout.strip().splitlines()[-1])
    print(json.dumps(res), flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
