#!/usr/bin/env python3
"""Generates tests/golden/refdiff.expected.json.gz: the REFERENCE's outputs on the random cases of tools/diff_ref.py (seeds
7000-7003: run_detect's segment TSV and --graph trees per window) and tools/diff_ref_predict.py (seeds 7100-7102: Predict.run's
.vcf / .score.txt per chromosome with a random classifier, the score list, merge_split_vcfs' merged VCF), each case stored with
the simulation config and options that make it, and the classifier outputs the reference consumed.  tests/test_reference_diff.py
runs the product's side of the same cases against it.  Same case draws as the two tools; needs the reference sources (refdriver)."""
import base64
import gzip
import json
import os
import shutil
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (before the stub modules are installed)
import refdriver  # noqa: E402

refdriver.install_stubs()
from src.collection import run_collection as ref_run  # noqa: E402
from src.network.output import cal_scores_max_min as ref_scores, merge_split_vcfs as ref_merge  # noqa: E402
from src.network.predict import Predict as RefPredict  # noqa: E402
from svision_amd import synth  # noqa: E402
from svision_amd.collection.output_clusters import collect_pair_lines  # noqa: E402
from svision_amd.collection.run_collection import detect_window  # noqa: E402
from svision_amd.io import bam  # noqa: E402
from svision_amd.sample import Sample  # noqa: E402
from tests import helpers  # noqa: E402
from tools.diff_ref import MIXES  # noqa: E402

COLLECT_SEEDS = range(7000, 7004)
PREDICT_SEEDS = range(7100, 7103)


def arr(a):
    a = np.ascontiguousarray(a)
    return {"dtype": a.dtype.str, "shape": list(a.shape), "b64": base64.b64encode(a.tobytes()).decode()}


def read_tree(gdir):
    tree = {}
    if os.path.exists(gdir):
        for d, _dirs, files in os.walk(gdir):
            for name in files:
                with open(os.path.join(d, name)) as f:
                    tree[os.path.relpath(os.path.join(d, name), gdir)] = f.read()
        shutil.rmtree(gdir)
    os.mkdir(gdir)
    return tree


def collect_case(seed):
    """tools/diff_ref.py one_case's draws and reference side."""
    rng = np.random.default_rng(seed)
    n_contigs = int(rng.integers(1, 4))
    contigs = [("c%d" % i, int(rng.integers(120_000, 420_000))) for i in range(n_contigs)]
    lognormal = bool(rng.random() < 0.3)
    cfg = dict(contigs=contigs, coverage=float(rng.choice([6, 10, 16, 24])),
               read_len_mean=float(rng.choice([3000, 6000, 9000, 14000])), read_len_sd=float(rng.choice([500, 1500, 3000])),
               lognormal=lognormal, err_rate=float(rng.choice([0.0, 0.002, 0.01, 0.04])),
               sv_spacing=float(rng.choice([3000, 6000, 12000])), sv_min_gap=int(rng.choice([2000, 5000, 9000])),
               sv_max=int(rng.choice([800, 4000, 20000])), inline_max=int(rng.choice([300, 1500, 4000])),
               het_frac=float(rng.choice([0.0, 0.5, 1.0])), seed=int(seed), sv_mix=MIXES[int(rng.integers(0, len(MIXES)))])
    use_hash = bool(rng.random() < 0.2)
    use_graph = bool(rng.random() < 0.25)
    table, genome, _svs = synth.simulate(synth.SimConfig(**cfg), with_seq=use_hash or use_graph)
    over = dict(hash=use_hash, graph=use_graph, min_support=int(rng.choice([1, 2, 3, 5, 8])), min_mapq=int(rng.choice([0, 10, 20, 40])),
                min_sv_size=int(rng.choice([30, 50, 100])), max_sv_size=int(rng.choice([3000, 1000000])),
                patition_max_distance=int(rng.choice([500, 5000])), cluster_max_distance=float(rng.choice([0.1, 0.3, 0.6])),
                contig=bool(rng.random() < 0.15), qname=bool(rng.random() < 0.2))
    window = int(rng.choice([60_000, 150_000, 10_000_000]))
    if over["contig"]:
        over["min_support"] = 1
    out = tempfile.mkdtemp()
    windows = []
    try:
        genome_path = os.path.join(out, "genome.fa")
        bam.write_fasta(genome_path, genome)
        refdriver.FASTAS.clear()
        refdriver.DATASETS.clear()
        refdriver.FASTAS[genome_path] = genome
        refdriver.DATASETS["sample.bam"] = table
        os.mkdir(os.path.join(out, "segments"))
        gdir = os.path.join(out, "graphs")
        read_tree(gdir)
        ropts = refdriver.default_options(out_path=out, genome=genome_path, bam_path="sample.bam", window_size=window, **over)
        for chrom, clen in contigs:
            part, pos = 0, 0
            while pos < clen:
                end = clen if over["contig"] else min(clen, pos + window)
                err = ref_run.run_detect(ropts, "sample.bam", chrom, part, pos, end)
                path = os.path.join(out, "segments", "%s.segments.%d.bed" % (chrom, part))
                want = open(path).read() if os.path.exists(path) else None
                if os.path.exists(path):
                    os.remove(path)
                windows.append({"chrom": chrom, "part": part, "start": pos, "end": end, "ref_error": err is not None,
                                "tsv": want, "graphs": read_tree(gdir) if use_graph else None})
                part += 1
                pos = end
    finally:
        shutil.rmtree(out)
    return {"seed": seed, "sim": cfg, "with_seq": use_hash or use_graph, "options": over, "window": window, "windows": windows}


def predict_case(seed):
    """tools/diff_ref_predict.py one_case's draws and reference side (the segment TSVs are the product's collection, as there)."""
    rng = np.random.default_rng(seed)
    contigs = [("c%d" % i, int(rng.integers(150_000, 380_000))) for i in range(int(rng.integers(1, 4)))]
    cfg = dict(contigs=contigs, coverage=float(rng.choice([8, 14, 22])), read_len_mean=float(rng.choice([5000, 9000])),
               read_len_sd=1500.0, err_rate=float(rng.choice([0.0, 0.004])), sv_spacing=float(rng.choice([4000, 9000])),
               sv_min_gap=int(rng.choice([3000, 8000])), sv_max=int(rng.choice([1500, 6000])), inline_max=int(rng.choice([500, 1500])),
               het_frac=float(rng.choice([0.0, 0.5, 1.0])), seed=int(seed), sv_mix=MIXES[int(rng.integers(0, len(MIXES)))])
    table, genome, _svs = synth.simulate(synth.SimConfig(**cfg))
    over = dict(min_support=int(rng.choice([1, 2, 3, 5])), batch_size=int(rng.choice([1, 7, 64, 128])), qname=bool(rng.random() < 0.3),
                min_gt_depth=int(rng.choice([1, 4, 10])), homo_thresh=float(rng.choice([0.6, 0.8])), hete_thresh=float(rng.choice([0.2, 0.35])),
                max_sv_size=int(rng.choice([2000, 1000000])), sample="S%d" % seed)
    window = int(rng.choice([100_000, 10_000_000]))
    sharp = float(rng.choice([0.3, 2.0, 6.0]))
    case = {"seed": seed, "sim": cfg, "options": over, "window": window, "chroms": []}
    out = tempfile.mkdtemp()
    try:
        genome_path = os.path.join(out, "genome.fa")
        bam.write_fasta(genome_path, genome)
        refdriver.FASTAS.clear()
        refdriver.DATASETS.clear()
        refdriver.FASTAS[genome_path] = genome
        refdriver.DATASETS["sample.bam"] = table
        seg_dir, rdir = os.path.join(out, "segments"), os.path.join(out, "ref_pred")
        os.mkdir(seg_dir)
        os.mkdir(rdir)
        ropts = refdriver.default_options(out_path=out, genome=genome_path, bam_path="sample.bam", window_size=window,
                                          model_path="unused.ckpt", **over)
        popts = helpers.default_options(out_path=out, genome=genome_path, bam_path="sample.bam", window_size=window,
                                        source_version="1.4", **over)
        fasta = bam.Fasta(sequences=genome)
        scan = helpers.oracle_scan(table, 50)
        chroms = []
        for chrom, clen in contigs:
            text, part, pos = "", 0, 0
            while pos < clen:
                end = min(clen, pos + window)
                _s, clusters = detect_window(popts, Sample.with_scan(table, fasta, 50, scan), chrom, pos, end, part)
                text += "".join(p.text() for p in collect_pair_lines(clusters, popts))
                part += 1
                pos = end
            if text:
                chroms.append(chrom)
                with open(os.path.join(seg_dir, chrom + ".segments.all.bed"), "w") as f:
                    f.write(text)
        if not chroms:
            return case
        for n, chrom in enumerate(chroms):
            crng = np.random.default_rng(seed * 1000 + n)
            preds = []

            def fn(batch, preds=preds, crng=crng):
                k = np.asarray(batch).shape[0]
                logits = crng.standard_normal((k, 5)).astype(np.float32) * np.float32(sharp)
                e = np.exp(logits - logits.max(1, keepdims=True))
                prob = (e / e.sum(1, keepdims=True)).astype(np.float32)
                cl = logits.argmax(1)
                preds.append((cl.copy(), prob.copy()))
                return logits, cl, prob
            refdriver.PREDICTOR["fn"] = fn
            rprefix = os.path.join(rdir, "%s.predict.s%d" % (chrom, over["min_support"]))
            RefPredict(chrom, os.path.join(seg_dir, chrom + ".segments.all.bed")).run(rprefix, ropts)
            case["chroms"].append({"chrom": chrom, "preds": [[arr(c.astype(np.int64)), arr(p)] for c, p in preds],
                                   "vcf": open(rprefix + ".vcf").read(), "score": open(rprefix + ".score.txt").read()})
        rs = ref_scores(rdir)
        case["scores"] = [float(x) for x in rs]
        if len(rs):
            ref_merge(rdir, os.path.join(out, "ref.vcf"), np.max(rs), np.min(rs), chroms, ropts)
            case["merged_vcf"] = open(os.path.join(out, "ref.vcf")).read()
    finally:
        shutil.rmtree(out)
    return case


if __name__ == "__main__":
    fixture = {"collection": [collect_case(s) for s in COLLECT_SEEDS], "predict": [predict_case(s) for s in PREDICT_SEEDS]}
    with gzip.open(os.path.join(HERE, "refdiff.expected.json.gz"), "wt") as f:
        json.dump(fixture, f, sort_keys=True)
    print("collection windows %d (TSV lines %d), predict chromosomes %d" % (
        sum(len(c["windows"]) for c in fixture["collection"]),
        sum((w["tsv"] or "").count("\n") for c in fixture["collection"] for w in c["windows"]),
        sum(len(c["chroms"]) for c in fixture["predict"])))
