"""The seven grouped launches of one decoder level's prediction heads (monodetr/heads.py: three NT forward groups, three NN input
gradient groups, the TN weight-gradient group) at T = 4 400 and T = 8 800 rows, each timed in both forms of csrc/sgemm.hip: the exact
f32-input instruction and the three-way bf16 split (MDETR_SGEMM_SPLIT).

Timing as tools/gemmbench.py: `reps` launches captured into one hipGraph and replayed, operands rotating over enough sets to exceed
the 256 MB Infinity Cache; microseconds per launch, the median of --repeats graph timings with [min, max].  JSON on stdout.

    python -m monodetr_amd.tools.headsbench [--rows 4400,8800] [--reps 24] [--repeats 3] [--x-dtype bf16]
"""
import argparse
import json
import os

import monodetr_amd._runtime_env  # noqa: F401  (before torch)
import torch

from .gemmbench import graph_time

LAUNCHES = ("nt1_first_layers_and_class", "nt2_second_layers", "nt3_256to6", "nn1_gdelta_w3b", "nn2_dh1", "nn3_dx", "tn_weight_gradients")


def level_sets(T, nsets, x_dtype, dev):
    """`nsets` independent operand sets of a level + one set of weights; -> launch(name, i, split)."""
    from monodetr_amd import sgemm_ext as S
    gen = torch.Generator(device="cpu").manual_seed(T)
    r = lambda *s: torch.randn(*s, generator=gen).to(dev)                           # noqa: E731
    hid = 256
    w1, b1 = [r(hid, hid) * 0.06 for _ in range(4)], [r(hid) for _ in range(4)]
    w2 = [r(hid, hid) * 0.06, r(3, hid), r(2, hid), r(24, hid)]
    b2 = [r(hid), r(3), r(2), r(24)]
    w3b, b3b, wc, bc = r(6, hid), r(6), r(3, hid), r(3)
    sl = [slice(i * hid, (i + 1) * hid) for i in range(4)]
    new = lambda *s, **k: torch.empty(*s, device=dev, **k)                          # noqa: E731
    sets = []
    for _ in range(nsets):
        d = dict(x=r(T, hid).to(x_dtype), h1=r(T, 4 * hid).clamp(min=0), h2=r(T, hid).clamp(min=0), dh1=r(T, 4 * hid), dh2=r(T, hid),
                 g=[r(T, 6), r(T, 3), r(T, 2), r(T, 24), r(T, 3)], skip=r(T, hid).to(x_dtype),
                 o_h1=new(T, 4 * hid), o_logits=new(T, 3), o2=[new(T, hid), new(T, 3), new(T, 2), new(T, 24)], o_delta=new(T, 6),
                 o_dh2=new(T, hid), o_dh1=new(T, 4 * hid), o_dx=new(T, hid, dtype=x_dtype))
        d["dw"] = [new(6, hid), new(hid, hid), new(3, hid), new(2, hid), new(24, hid)] + [new(hid, hid) for _ in range(4)] + [new(3, hid)]
        d["db"] = [new(w.shape[0]) for w in d["dw"]]
        sets.append(d)
    P = S.Problem

    def launch(name, i, split):
        d = sets[i]
        g_delta, g_size, g_depth, g_angle, g_logits = d["g"]
        if name == LAUNCHES[0]:
            S.grouped(S.NT, [P([(d["x"], w)], d["o_h1"][:, s], bias=b, relu_cols=True) for w, b, s in zip(w1, b1, sl)]
                      + [P([(d["x"], wc)], d["o_logits"], bias=bc)], split=split)
        elif name == LAUNCHES[1]:
            S.grouped(S.NT, [P([(d["h1"][:, s], w)], o, bias=b, relu_cols=(True if j == 0 else 0))
                             for j, (s, w, b, o) in enumerate(zip(sl, w2, b2, d["o2"]))], split=split)
        elif name == LAUNCHES[2]:
            S.grouped(S.NT, [P([(d["h2"], w3b)], d["o_delta"], bias=b3b)], split=split)
        elif name == LAUNCHES[3]:
            S.grouped(S.NN, [P([(g_delta, w3b)], d["o_dh2"], mask=d["h2"])], split=split)
        elif name == LAUNCHES[4]:
            S.grouped(S.NN, [P([(g, w)], d["o_dh1"][:, s], mask=d["h1"][:, s]) for g, w, s in zip((d["dh2"], g_size, g_depth, g_angle), w2, sl)],
                      split=split)
        elif name == LAUNCHES[5]:
            S.grouped(S.NN, [P([(d["dh1"][:, s], w) for s, w in zip(sl, w1)] + [(g_logits, wc)], d["o_dx"], res=d["skip"])], split=split)
        else:
            ops = [(g_delta, d["h2"]), (d["dh2"], d["h1"][:, sl[0]]), (g_size, d["h1"][:, sl[1]]), (g_depth, d["h1"][:, sl[2]]),
                   (g_angle, d["h1"][:, sl[3]])] + [(d["dh1"][:, s], d["x"]) for s in sl] + [(g_logits, d["x"])]
            S.grouped(S.TN, [P([op], dw, colsum=db) for op, dw, db in zip(ops, d["dw"], d["db"])], split=split)
    return launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="4400,8800")
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--x-dtype", default="bf16", choices=("bf16", "fp32"), help="the level's input (bf16: the bf16 body of the measured step)")
    ap.add_argument("--only", default="")
    ap.add_argument("--variants", default="", help="the split form again under these MDETR_TUNE strings, 'sgemm_split_tm=64;sgemm_split_images=1,...'")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    x_dtype = torch.bfloat16 if a.x_dtype == "bf16" else torch.float32
    res = {"device": torch.cuda.get_device_name(0), "x_dtype": a.x_dtype, "reps": a.reps, "repeats": a.repeats, "unit": "us per launch", "rows": {}}
    for T in [int(t) for t in a.rows.split(",")]:
        nsets = 6                                                    # ~55 MB of operands and results per set at T = 4 400
        launch = level_sets(T, nsets, x_dtype, dev)
        table = {}
        for name in LAUNCHES:
            if a.only and not any(k in name for k in a.only.split(",")):
                continue
            row = {}
            for form, split in (("exact", False), ("split", True)):
                ts = sorted(graph_time(lambda i: launch(name, i, split), nsets, a.reps) for _ in range(a.repeats))
                row[form] = {"median": ts[len(ts) // 2], "min": ts[0], "max": ts[-1]}
            row["split_faster_than_exact_min"] = row["split"]["max"] < row["exact"]["min"]
            for var in [v for v in a.variants.split(";") if v]:
                os.environ["MDETR_TUNE"] = var
                ts = sorted(graph_time(lambda i: launch(name, i, True), nsets, a.reps) for _ in range(a.repeats))
                row["split[%s]" % var] = {"median": ts[len(ts) // 2], "min": ts[0], "max": ts[-1]}
                os.environ.pop("MDETR_TUNE", None)
            table[name] = row
        table["total"] = {form: round(sum(r[form]["median"] for r in table.values()), 2) for form in next(iter(table.values()))
                          if form != "split_faster_than_exact_min"}
        res["rows"][str(T)] = table
        del launch
        torch.cuda.empty_cache()
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
