"""Differential check against the reference's own outputs: random samples and option sets (the cases of tools/diff_ref.py,
seeds 7000-7003, and tools/diff_ref_predict.py, seeds 7100-7102) through the product's host code, compared byte for byte with
what the reference's run_detect / Predict.run / merge_split_vcfs wrote for them (tests/golden/refdiff.expected.json.gz, made by
tests/golden/make_refdiff_fixture.py; the prediction cases carry the classifier outputs the reference consumed).
tools/diff_ref*.py take a seed range for longer runs against the reference itself (580 collection cases / 230,000 TSV lines
and 230 prediction cases were compared that way in round 1)."""
import base64
import gzip
import json
import os
import shutil

import numpy as np
import pytest

from svision_amd import synth
from svision_amd.collection.output_clusters import collect_pair_lines
from svision_amd.collection.run_collection import detect_window
from svision_amd.io import bam
from svision_amd.network import output
from svision_amd.network.predict import Predict
from svision_amd.sample import Sample
from tests import helpers


@pytest.fixture(scope="module")
def fixture():
    with gzip.open(os.path.join(helpers.GOLDEN, "refdiff.expected.json.gz"), "rt") as f:
        return json.load(f)


def _arr(d):
    return np.frombuffer(base64.b64decode(d["b64"]), dtype=np.dtype(d["dtype"])).reshape(d["shape"])


def _sim(case, with_seq=False):
    cfg = dict(case["sim"])
    cfg["contigs"] = [tuple(c) for c in cfg["contigs"]]
    cfg["sv_mix"] = tuple(tuple(m) for m in cfg["sv_mix"])
    return synth.simulate(synth.SimConfig(**cfg), with_seq=with_seq)[:2]


def _read_tree(gdir):
    tree = {}
    if os.path.exists(gdir):
        for d, _dirs, files in os.walk(gdir):
            for name in files:
                with open(os.path.join(d, name)) as f:
                    tree[os.path.relpath(os.path.join(d, name), gdir)] = f.read()
        shutil.rmtree(gdir)
    os.mkdir(gdir)
    return tree


def test_collection_equals_reference_on_random_samples(fixture, oracle_lib, tmp_path):
    lines = 0
    for case in fixture["collection"]:
        over = case["options"]
        table, genome = _sim(case, case["with_seq"])
        out = tmp_path / ("c%d" % case["seed"])
        out.mkdir()
        genome_path = str(out / "genome.fa")
        bam.write_fasta(genome_path, genome)
        gdir = str(out / "graphs")
        _read_tree(gdir)
        popts = helpers.default_options(out_path=str(out), genome=genome_path, bam_path="sample.bam", window_size=case["window"], **over)
        fasta = bam.Fasta(sequences=genome)
        scan = helpers.oracle_scan(table, over["min_sv_size"])
        for w in case["windows"]:
            where = "seed %d %s:%d-%d" % (case["seed"], w["chrom"], w["start"], w["end"])
            sample = Sample.with_scan(table, fasta, over["min_sv_size"], scan)
            try:                                             # run_detect's catch-all: a failing window writes nothing
                _sigs, clusters = detect_window(popts, sample, w["chrom"], w["start"], w["end"], w["part"])
                got = "".join(p.text() for p in collect_pair_lines(clusters, popts))
            except Exception as exc:                         # noqa: BLE001
                assert w["ref_error"], "product-only exception %s: %r" % (where, exc)
                got = ""
            got_graphs = _read_tree(gdir)
            if over["graph"] and not w["ref_error"]:
                assert got_graphs == w["graphs"], "graph trees differ " + where
            assert got == (w["tsv"] or ""), "TSV differs " + where
            lines += got.count("\n")
    assert lines > 200                                       # TSV lines compared


class Injected:
    needs_images = False

    def __init__(self, preds):
        self.preds, self.i = preds, 0

    def __call__(self, _images):
        cl, pr = self.preds[self.i]
        self.i += 1
        return None, cl, pr


def test_vote_vcf_merge_equal_reference_on_random_samples(fixture, oracle_lib, tmp_path):
    records = 0
    for case in fixture["predict"]:
        over = case["options"]
        table, genome = _sim(case)
        out = tmp_path / ("p%d" % case["seed"])
        seg_dir, pdir = out / "segments", out / "own_pred"
        seg_dir.mkdir(parents=True)
        pdir.mkdir()
        genome_path = str(out / "genome.fa")
        bam.write_fasta(genome_path, genome)
        popts = helpers.default_options(out_path=str(out), genome=genome_path, bam_path="sample.bam", window_size=case["window"],
                                        source_version="1.4", **over)
        fasta = bam.Fasta(sequences=genome)
        scan = helpers.oracle_scan(table, 50)
        chroms = []
        for chrom, clen in case["sim"]["contigs"]:
            text, part, pos = "", 0, 0
            while pos < clen:
                end = min(clen, pos + case["window"])
                _s, clusters = detect_window(popts, Sample.with_scan(table, fasta, 50, scan), chrom, pos, end, part)
                text += "".join(p.text() for p in collect_pair_lines(clusters, popts))
                part += 1
                pos = end
            if text:
                chroms.append(chrom)
                (seg_dir / (chrom + ".segments.all.bed")).write_text(text)
        assert chroms == [c["chrom"] for c in case["chroms"]], case["seed"]
        sample = Sample.with_scan(table, fasta, 50, scan)
        for c in case["chroms"]:
            prefix = str(pdir / ("%s.predict.s%d" % (c["chrom"], over["min_support"])))
            preds = [(_arr(cl), _arr(pr)) for cl, pr in c["preds"]]
            Predict(c["chrom"], str(seg_dir / (c["chrom"] + ".segments.all.bed"))).run(prefix, popts, classifier=Injected(preds), sample=sample)
            assert open(prefix + ".vcf").read() == c["vcf"], "seed %d %s.vcf" % (case["seed"], c["chrom"])
            assert open(prefix + ".score.txt").read() == c["score"], "seed %d %s.score.txt" % (case["seed"], c["chrom"])
            records += c["vcf"].count("\n")
        if not chroms:
            continue
        ps = output.cal_scores_max_min(str(pdir))
        assert [float(x) for x in ps] == case["scores"], case["seed"]
        if len(ps):
            output.merge_split_vcfs(str(pdir), str(out / "own.vcf"), np.max(ps), np.min(ps), chroms, popts, fasta=fasta)
            assert (out / "own.vcf").read_text() == case["merged_vcf"], "seed %d merged VCF" % case["seed"]
    assert records > 20                                      # VCF records compared
