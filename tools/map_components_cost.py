#!/usr/bin/env python3
"""Development tool: what the component labelling of the map costs on the bench-shaped jobs, and what the component vote does to the
cloud verdict -- scvod_map_components and scvod_map_component_visibility (csrc/scvod_mapcomp.hip) on the representatives of the batch's
labelled map, next to scvod_map_query (csrc/scvod_mapquery.hip, the parent commit's kernel) of the same representatives at radius
0.99 * leaf with d_result and the nn pair as the yardstick: the query walks the own cell and probes 26 neighbours per point, pass 2 of
the labelling probes 13, and adds the union-find, the flatten, the reduction, a sort of n pairs and the ranking.
The map: every input point of the batch, 0.2 m cells, label byte = bit 0 truth-moving (label & 0xFFFF in 252..259, as
tools/cloud_visibility_cost.py takes it), bit 1 truth-ground (the synthetic plane, class 40 -- a stand-in for the recognised map's
label 1).  Two lists: `all` = every cell, `ng` = the cells whose label has no ground bit (points_labelled with a select table).
One process per job; on one processed batch, timed in interleaved rounds:
  c26_all c18_all c6_all c26_ng c18_ng c6_ng   components: d_component + table + d_n
  label_all label_ng                           connectivity 26 with d_n alone: slots, init, union, flatten -- no reduction, sort, ranking
  vote_ng                                      scvod_map_component_visibility of the ng list: defaults, votes, records, verdict
  query_all query_ng                           scvod_map_query, radius 0.99 * leaf, d_result + d_nn_key + d_nn_sqdist
Stream-event times; the median, minimum and maximum of --reps rounds after --warmup rounds.  `spread` of a row is (max - min) / median.
The same run counts, on these SYNTHETIC jobs, the truth-moving and the other cells of the ng list that the cloud verdict
(scvod_cloud_visibility_device, defaults, all scans) flags, and that remain flagged behind the component vote with the defaults, with
SCVOD_CMPVIS_POOL_PAIRS, and with max_cells = 4096; the largest component and the share of cells in components above 4096 records.
Recorded, not asserted; no statement about real data.  No hardware counters.  Writes one block per job to
profiles/map_components_cost.txt.
usage: python tools/map_components_cost.py [--jobs K64,PARK,OS128] [--scale 1.0] [--reps 7] [--warmup 2] [--note TEXT]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dr-using-scv-od_amd", "pyshim"))

JOBS = {"K64": ("semantickitti", 5, 2761, 5), "PARK": ("parkinglot", 3, 2000, 1), "OS128": ("os128_fine", 5, 1000, 5)}
OUT = os.path.join(ROOT, "profiles", "map_components_cost.txt")
LEAF = 0.2
BIG = 4096


def summary(ms):
    med = float(np.median(ms))
    return dict(ms=round(med, 3), ms_min=round(float(min(ms)), 3), ms_max=round(float(max(ms)), 3),
                spread=round((max(ms) - min(ms)) / max(med, 1e-9), 3))


def run(kind, scale, reps, warmup):
    import torch
    import scvod_py
    import synth
    preset, seq, count, skip = JOBS[kind]
    count = max(skip + 1, int(count * scale))
    P = scvod_py.make_params(preset)
    scans = [synth.make_scan(seq, i, kind, device="cuda") for i in range(count)]
    d = torch.cat([s[0] for s in scans]).contiguous()
    labels = torch.cat([s[1] for s in scans]).contiguous()
    offs = np.concatenate([[0], np.cumsum([len(s[0]) for s in scans])]).astype(np.int32)
    poses = np.asarray([s[2] for s in scans], np.float32)
    del scans
    n = int(offs[-1])
    print(f"{kind}: {count} scans, {n} points", file=sys.stderr, flush=True)
    ctx = scvod_py.Ctx(P, max_points_total=n + 64, max_scans=count)
    nxt = np.asarray([s + skip if s + skip < count else -1 for s in range(count)], np.int32)
    st = torch.cuda.current_stream().cuda_stream
    ctx.batch_process(d, offs, stream=st, sync=False)
    torch.cuda.synchronize()
    cls = labels.to(torch.int64) & 0xFFFF
    byte = ((cls >= 252) & (cls <= 259)).to(torch.uint8) + 2 * (cls == 40).to(torch.uint8)
    del cls, labels
    images = ctx.batch_visibility(poses, nxt, flags=scvod_py.VIS_WITH_GROUND, want=("verdict", "images"), stream=st)["images"]
    cells = 1 << int(np.ceil(np.log2(max(n * 0.25, 1 << 22))))       # the benchmark's sizing
    raw = scvod_py.StaticMap(cells, leaf=LEAF, kind=scvod_py.MAP_KIND_LABELLED)
    raw.accumulate_labelled(d, byte, offs, poses, stream=st)
    lists = {}
    for name, select in (("all", None), ("ng", [0, 1])):
        pts, lab, recs = raw.points_labelled(select=select, stream=st)
        lists[name] = (pts.contiguous(), lab.contiguous(), recs.contiguous())
    torch.cuda.synchronize()
    del d, byte
    sizes = {k: int(v[0].shape[0]) for k, v in lists.items()}
    print(f"{kind}: {sizes} map points", file=sys.stderr, flush=True)
    lib, C = raw.lib, scvod_py.C
    vp = C.c_void_p

    def p(t):
        return vp(t.data_ptr())

    buf = {}
    for name, (pts, lab, recs) in lists.items():
        m = sizes[name]
        buf[name] = dict(comp=torch.empty(m, dtype=torch.int32, device="cuda"), table=torch.empty((m, 48), dtype=torch.uint8, device="cuda"),
                         n=torch.zeros(1, dtype=torch.int64, device="cuda"), result=torch.empty(m, dtype=torch.uint8, device="cuda"),
                         nn_key=torch.empty(m, dtype=torch.int64, device="cuda"), nn_sq=torch.empty(m, dtype=torch.float32, device="cuda"),
                         off=np.asarray([0, m], np.int32))
    m_ng = sizes["ng"]
    pts_ng = lists["ng"][0]
    cv = ctx.cloud_visibility(pts_ng, images, poses, stream=st)
    verdict, votes = cv["verdict"], cv["votes"]
    vrec = torch.empty((m_ng, 64), dtype=torch.uint8, device="cuda")
    vout = torch.empty(m_ng, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def comp(name, conn, full=True):
        b, recs = buf[name], lists[name][2]
        rc = lib.scvod_map_components(raw.h, p(recs), sizes[name], conn, p(b["comp"]) if full else None, p(b["table"]) if full else None,
                                      sizes[name] if full else 0, p(b["n"]), vp(st))
        assert rc == 0, lib.scvod_map_last_error(raw.h).decode()

    def vote(prm=None):
        b = buf["ng"]
        rc = lib.scvod_map_component_visibility(raw.h, p(b["comp"]), m_ng, p(b["n"]), m_ng, p(verdict), p(votes), C.byref(prm) if prm else None,
                                                p(vrec), m_ng, p(vout), vp(st))
        assert rc == 0, lib.scvod_map_last_error(raw.h).decode()

    def query(name):
        b = buf[name]
        rc = lib.scvod_map_query(raw.h, p(lists[name][0]), b["off"].ctypes.data_as(vp), 1, None, 0.99 * LEAF, None, p(b["result"]), None,
                                 p(b["nn_key"]), p(b["nn_sq"]), None, vp(st))
        assert rc == 0, lib.scvod_map_last_error(raw.h).decode()

    arms = [("c%d_%s" % (conn, name), (lambda name=name, conn=conn: comp(name, conn))) for name in ("all", "ng") for conn in (26, 18, 6)]
    arms += [("label_all", lambda: comp("all", 26, False)), ("label_ng", lambda: comp("ng", 26, False))]
    arms += [("c26_ng_for_vote", lambda: comp("ng", 26)), ("vote_ng", vote), ("query_all", lambda: query("all")), ("query_ng", lambda: query("ng"))]
    ms = {name: [] for name, _ in arms}
    stats = {}
    for r in range(warmup + reps):
        print(f"{kind}: round {r}", file=sys.stderr, flush=True)
        for name, fn in arms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= warmup:
                ms[name].append(e0.elapsed_time(e1))
            if r == 0 and name.startswith("c"):
                stats[name] = raw.components_stats()
    out = dict(kind=kind, scans=count, input_points=n, map_slots=cells, cells=sizes, components_scratch_bytes=raw.components_scratch_bytes())
    for name in ms:
        if name != "c26_ng_for_vote":
            out[name] = summary(ms[name])
    out["stats"] = {k: v for k, v in stats.items() if k != "c26_ng_for_vote"}
    out["c26_over_query"] = {k: round(out["c26_" + k]["ms"] / max(out["query_" + k]["ms"], 1e-9), 3) for k in ("all", "ng")}
    out["label_share_of_c26"] = {k: round(out["label_" + k]["ms"] / max(out["c26_" + k]["ms"], 1e-9), 3) for k in ("all", "ng")}
    # the sizes: the largest component, the share of records in components above BIG
    shapes = {}
    for name in ("all", "ng"):
        comp(name, 26)
        torch.cuda.synchronize()
        nc = int(buf[name]["n"].item())
        nrec = buf[name]["table"][:nc].cpu().numpy().view(scvod_py.MAP_COMPONENT_DTYPE)["n_records"].reshape(-1).astype(np.int64)
        shapes[name] = dict(components=nc, largest=int(nrec.max()) if nc else 0, singletons=int((nrec == 1).sum()),
                            share_above_4096=round(float(nrec[nrec > BIG].sum()) / max(sizes[name], 1), 5))
    out["shapes_26"] = shapes
    # what the vote does to the cloud verdict of the ng list (buf["ng"] holds the connectivity-26 labelling of it)
    lab = lists["ng"][1]
    mov = (lab & 1) != 0

    def c(t):
        return int(t.sum().item())
    seen = verdict == scvod_py.VIS_SEEN_THROUGH
    flags = dict(moving_cells=c(mov), static_cells=c(~mov), before=dict(moving=c(mov & seen), static=c(~mov & seen)))
    for arm, kw in (("defaults", {}), ("pool_pairs", dict(flags=scvod_py.CMPVIS_POOL_PAIRS)), ("max_cells_4096", dict(max_cells=BIG))):
        vote(scvod_py.component_visibility_params_default(**kw))
        torch.cuda.synchronize()
        s = vout == scvod_py.VIS_SEEN_THROUGH
        flags[arm] = dict(moving=c(mov & s), static=c(~mov & s), stats=raw.component_visibility_stats())
    out["flags"] = flags
    raw.close()
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", default="K64,PARK,OS128")
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the bench job's scans")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--note", default="", help="a line for the head of the file (e.g. the build that was measured)")
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--child", default="", help="internal: run this one job and print its line")
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(run(a.child, a.scale, a.reps, a.warmup)), flush=True)
        return
    head = ("Components of the map (scvod_map_components, scvod_map_component_visibility; csrc/scvod_mapcomp.hip): cost and effect on the bench-shaped jobs\n"
            f"written by tools/map_components_cost.py --jobs {a.jobs} --scale {a.scale} --reps {a.reps} --warmup {a.warmup}\n"
            + (a.note + "\n" if a.note else "") +
            "per job, one process, on one processed batch, interleaved rounds.  The map: every input point, 0.2 m cells, label bit 0 truth-moving\n"
            "(label & 0xFFFF in 252..259), bit 1 truth-ground (the synthetic plane, class 40; a stand-in for the recognised map's label 1).\n"
            "Lists: all = every cell, ng = cells without the ground bit (points_labelled with a select table), both in table-slot order.\n"
            "  c26 / c18 / c6_<list>  scvod_map_components: d_component + table + d_n\n"
            "  label_<list>           connectivity 26 with d_n alone: slots, init, union, flatten; no reduction, sort or ranking\n"
            "  vote_ng                scvod_map_component_visibility, defaults, with d_votes, records and d_verdict_out\n"
            "  query_<list>           scvod_map_query of the same representatives, radius 0.99 * leaf, d_result + nn pair (the parent commit's kernel)\n"
            "ms = median of the stream-event times after the warm-up rounds, with minimum, maximum and spread = (max - min) / median.\n"
            "c26_over_query: the aim is <= 1.  label_share_of_c26: the share of c26 that the four labelling passes take; the rest is the\n"
            "reduction per root, the sort of n pairs, the ranking and d_component.  stats = scvod_map_components_stats of the arm.\n"
            "shapes_26: components, the largest one, singletons, the share of records in components above 4096 records.\n"
            "flags = cells of the ng list by the truth of their representative that carry SCVOD_VIS_SEEN_THROUGH: before = the cloud verdict\n"
            "(scvod_cloud_visibility_device, defaults, all scans), then behind the component vote (connectivity 26) with the defaults, with\n"
            "POOL_PAIRS, with max_cells = 4096; stats = scvod_map_component_visibility_stats.  Synthetic scans: recorded, not asserted, and no\n"
            "statement about real data.  No hardware counters were taken.  A job that is missing below was not measured.\n\n")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(head)
    for kind in a.jobs.split(","):
        # a process per job: a fresh device context, nothing left over from the job before
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", kind, "--scale", str(a.scale), "--reps", str(a.reps),
                            "--warmup", str(a.warmup)], stdout=subprocess.PIPE, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        line = f"{kind}: {lines[-1][7:]}" if r.returncode == 0 and lines else f"{kind}: failed with status {r.returncode}"
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
        if r.returncode != 0:   # (nothing more is started on a device a job has failed on)
            sys.exit(1)


if __name__ == "__main__":
    main()
