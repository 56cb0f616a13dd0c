"""Tier X through the native driver (cw_run_correction, consent_amd.pipeline.correct_reads): a read set in which several reads carry different random
insertions of 1 500-1 800 bases at one locus.  With 1 900-base windows (cw_configure(1900); the re-assembly takes windows of up to 2 048 - 2 x overlap) the window of such a read over the locus aligns a dozen
unrelated pieces of that length -- a POA task beyond tier G's cells -- which stopped the whole run before tier X existed ("engine capacity exceeded").
Now the driver's output equals the oracle's pipeline record for record; with tier X switched off (test aid CW_NO_TIER_X) the run stops again, and
on_capacity="skip" leaves out some of the reads across the locus -- every window of a read there holds pieces of the insertions -- and
nothing else: the reads that end before the locus or begin after it are corrected as before."""
import random

import pytest

import consent_amd as ca
from consent_amd.pipeline import correct_reads
from test_gpu_pipeline import noisy_map, oracle_pipeline
from test_oracle_ref import rand_seq

pytestmark = pytest.mark.gpu
PRM = dict(min_support=3, max_support=150, window_size=1900, mer_size=9, common_kmers=8, min_anchors=2, solid_thresh=4, window_overlap=50, max_msa=150)


def insertion_dataset(tmp_path, seed, n_reads=18, glen=5000, locus=2500, n_ins=10, n_side=8):
    """make_dataset's construction (noisy copies of a random genome, overlaps from the genome coordinates, forward strand): `n_reads` reads across
    `locus`, the first `n_ins` of them with a random insertion of 1 500-1 800 bases there, and `n_side` reads that end 200 bases before the locus
    or begin 200 bases after it."""
    rng = random.Random(seed)
    genome = rand_seq(rng, glen)
    reads = []
    for i in range(n_reads + n_side):
        if i < n_reads:
            g0, g1 = rng.randrange(0, 600), rng.randrange(glen - 600, glen)
            left, pl = noisy_map(rng, genome[g0:locus], 0.04)
            right, pr = noisy_map(rng, genome[locus:g1], 0.04)
            ins = rand_seq(rng, rng.randrange(1500, 1801)) if i < n_ins else ""
            seq, pos = left + ins + right, pl[:-1] + [len(left) + len(ins) + p for p in pr]
        else:
            g0, g1 = (rng.randrange(0, 400), locus - 200) if i % 2 else (locus + 200, rng.randrange(glen - 400, glen))
            seq, pos = noisy_map(rng, genome[g0:g1], 0.04)
        reads.append(dict(name=f"r{i}", g0=g0, g1=g1, pos=pos, seq=seq, cross=i < n_reads))
    fa = tmp_path / "reads.fa"
    with open(fa, "w") as f:
        for r in reads:
            f.write(f">{r['name']} len={len(r['seq'])}\n{r['seq']}\n")
    paf = tmp_path / "ovl.paf"
    with open(paf, "w") as f:
        for q in reads:
            for t in reads:
                if t is q:
                    continue
                a, b = max(q["g0"], t["g0"]), min(q["g1"], t["g1"])
                if b - a < 400:
                    continue
                qs, qe = q["pos"][a - q["g0"]], q["pos"][b - q["g0"]]
                ts, te = t["pos"][a - t["g0"]], t["pos"][b - t["g0"]]
                f.write("\t".join(str(x) for x in [q["name"], len(q["seq"]), qs, qe, "+", t["name"], len(t["seq"]), ts, te, int((b - a) * 0.9), b - a, 60]) + "\n")
    return str(fa), str(paf), {r["name"] for r in reads if r["cross"]}


def test_reads_whose_windows_need_tier_x_are_corrected_like_the_oracle(tmp_path, aids, monkeypatch, capfd):
    fa, paf, across = insertion_dataset(tmp_path, 0x71E5)
    full = correct_reads(fa, paf, None, **PRM)
    want = oracle_pipeline(fa, paf, **PRM)
    assert [n for n, _ in full] == [n for n, _ in want]
    for (n, s), (_, w) in zip(full, want):
        assert s == w, f"read {n} differs from the oracle's pipeline"
    monkeypatch.setenv("CW_NO_TIER_X", "1")  # (the fixture `aids`: the test-aid build, in this process and in the driver)
    with pytest.raises(ca.EngineError, match="capacity"):
        correct_reads(fa, paf, None, **PRM)
    part = correct_reads(fa, paf, None, on_capacity="skip", **PRM)
    err = capfd.readouterr().err
    fd = dict(full)
    for n, s in part:
        assert fd[n] == s
    left_out = set(fd) - {n for n, _ in part}
    assert left_out and left_out <= across and len(part) >= 6, (sorted(left_out), sorted(across), len(part))
    for n in left_out:
        assert n in err
