"""FASTA in, corrected FASTA out, with no PAF from outside (pipeline.correct_from_reads): the overlaps found on the device, written as PAF and corrected by
cw_run_correction, give byte for byte the FASTA that cw_run_correction gives from a PAF written from the plain reference's rows (tests/overlap_probes.py)."""
import os

import pytest

import consent_amd as ca
import overlap_probes as op
import sw_op_probes as sp
from consent_amd import pipeline
from consent_amd.engine import SW_SCORE, write_paf

pytestmark = pytest.mark.gpu
FIND = dict(k=15, sample=0, min_hits=4)  # every k-mer: reads of 800 to 2 000 bases are shorter than OVL_MIN_OVERLAP, which the defaults are measured for


def corrected(run, out_path):
    with open(out_path, "wb") as f:
        run(f.fileno())
    return open(out_path, "rb").read()


def test_fasta_alone_gives_the_fasta_of_the_reference_rows(tmp_path):
    genome, reads, where = op.planted(*op.SMALL)
    names = [f"read{i}" for i in range(len(reads))]
    fasta, paf = str(tmp_path / "reads.fasta"), str(tmp_path / "reference.paf")
    with open(fasta, "w") as f:
        f.write("".join(f">{n}\n{r}\n" for n, r in zip(names, reads)))
    per = [e[2] for e in op.expected(reads, FIND["k"], FIND["sample"], 0, FIND["min_hits"])]
    assert write_paf(paf, names, [len(r) for r in reads], per) > 100
    want = corrected(lambda fd: pipeline.run_correction(fasta, paf, fd, devices=[0]), str(tmp_path / "want.fasta"))
    kept = str(tmp_path / "device.paf")
    got = corrected(lambda fd: pipeline.correct_from_reads(fasta, fd, paf_path=kept, **FIND), str(tmp_path / "got.fasta"))
    assert open(kept).read() == open(paf).read()  # the PAF the device's rows give is the reference's
    assert got == want and got.count(b">") >= 1
    again = corrected(lambda fd: pipeline.correct_from_reads(fasta, fd, **FIND), str(tmp_path / "again.fasta"))
    assert again == got and not [p for p in os.listdir(tmp_path) if p.endswith(".paf") and p not in ("reference.paf", "device.paf")]
    # measured, not asserted: how much closer to the genome the corrected reads are than the raw ones
    lines = got.decode().split("\n")
    fixed = {lines[i][1:]: lines[i + 1].upper() for i in range(0, len(lines) - 1, 2)}
    eng = ca.Engine(ca.Params(*sp.PRM))
    try:
        truth = {n: (op.revcomp(genome[a : a + m]) if turned else genome[a : a + m]) for n, (a, m, turned, _) in zip(names, where)}
        raw = eng.sw([[truth[n], r] for n, r in zip(names, reads) if n in fixed]).rows
        new = eng.sw([[truth[n], fixed[n]] for n in names if n in fixed]).rows
        print(f"{len(fixed)} of {len(reads)} reads corrected; summed local score against the true slice: raw {int(raw[1::2, SW_SCORE].sum())}, "
              f"corrected {int(new[1::2, SW_SCORE].sum())}; bases raw {sum(len(r) for n, r in zip(names, reads) if n in fixed)}, corrected {sum(len(v) for v in fixed.values())}")
    finally:
        eng.close()
