"""`python -m strkit_amd call <alignments.bam> --ref ref.fa --loci catalog.bed [--json out.json] [--realign]` — the
subset of `strkit call` (strkit/entry.py:20-342) that the device backend covers: per-read copy numbers per locus and, with
`--call-alleles`, a genotype per locus (`--consensus`: with the sequence of every allele, which a VCF with alleles needs;
`--consensus-method poa`: by partial-order alignment where the reads of an allele differ);
`--count-kmers`: the motif-sized k-mers of every tract, per read and per allele.
`--gff genes.gff3.gz`: the ids of the genome features every locus overlaps (`annotations`, `ANNOT` in the VCF).
`python -m strkit_amd mi <child> <mother> <father> [--caller strkit-json|strkit-vcf] [--test [x2|wmw|wmw-gt]]` — `strkit mi` over
the files `call` writes (strkit_amd/mi.py)."""
from __future__ import annotations

import argparse
import sys


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="strkit_amd")
    sub = ap.add_subparsers(dest="cmd", required=True)
    c = sub.add_parser("call", help="per-read repeat counts for every catalog locus")
    c.add_argument("read_file")
    c.add_argument("--ref", required=True)
    c.add_argument("--loci", required=True)
    c.add_argument("--json", default="-")
    c.add_argument("--vcf", default=None, help="also write the loci as VCF (read-level fields; with --call-alleles: alleles and genotypes, which switches --consensus on)")
    c.add_argument("--flank-size", type=int, default=70)
    c.add_argument("--min-avg-phred", type=int, default=13)
    c.add_argument("--max-reads", type=int, default=250)
    c.add_argument("--realign", action="store_true")
    c.add_argument("--front-end", choices=("auto", "device", "host"), default="auto",
                   help="where the alignment file is inflated, scanned and cut: on the GPU (whole below 24 GB: about six times the "
                        "file in device memory; larger files with a .bai in spans) or on the host cores, block by block through "
                        "the .bai; auto = device (a file of 24 GB or more needs its .bai for that)")
    c.add_argument("--span-mb", type=int, default=4096,
                   help="device front end, files of 24 GB and more: compressed megabytes of the file that go through device memory at a time")
    c.add_argument("--respect-ref", action="store_true")
    c.add_argument("--call-alleles", action="store_true", help="call a genotype per locus (GPU allele caller)")
    c.add_argument("--consensus", action="store_true",
                   help="with --call-alleles: report the sequence of every allele (single / best_rep, or poa with --consensus-method poa)")
    c.add_argument("--consensus-method", choices=("best_rep", "poa"), default="best_rep",
                   help="the sequence of an allele whose reads differ: its best representative read, or the consensus of its "
                        "reads by partial-order alignment (GPU)")
    c.add_argument("--max-mdn-poa-length", type=int, default=5000,
                   help="--consensus-method poa: an allele whose median read length is above this keeps its best representative")
    c.add_argument("--n-alleles", type=int, choices=(1, 2), default=2, help="alleles per locus, all contigs")
    c.add_argument("--ploidy", "--sex-chr", "-x", dest="ploidy", default=None, metavar="NAME|PATH",
                   help="ploidy configuration of the sample: haploid, diploid_autosomes, diploid_xx/XX, diploid_xy/XY, or a JSON file "
                        "(default, overrides per contig pattern, ignored contig patterns; up to 6 alleles).  Every contig is called "
                        "with its own number of alleles and loci on contigs without one are left out; replaces --n-alleles "
                        "(needs --call-alleles)")
    c.add_argument("--count-kmers", "-k", nargs="?", type=str, default="none", const="peak", choices=("none", "peak", "read", "both"),
                   help="count the motif-sized k-mers of every read's repeat tract (GPU): per read, summed per allele (peak; the "
                        "default when the flag stands alone; needs --call-alleles), or both")
    # same names as `strkit call` (strkit/entry.py:20-342); --seed seeds the allele caller (the per-read path has no random
    # component), --processes sizes the locus blocks as the reference does (loci.py:193)
    c.add_argument("--use-hp", action="store_true", help="group reads by their HP / PS tags where a locus has enough tagged reads (needs --call-alleles)")
    c.add_argument("--incorporate-snvs", "--snv", "-v", dest="incorporate_snvs", default=None, metavar="PATH",
                   help="VCF (plain or gzip; BGZF with a PATH.tbi next to it is read region by region) of candidate SNVs: reads are grouped by "
                        "the bases they carry at them (needs --call-alleles)")
    c.add_argument("--snv-phase-sets", action="store_true",
                   help="--incorporate-snvs: loci that share heterozygous SNVs get one phase set (PS, '|' genotypes), and the "
                        "called SNVs are written to the VCF as records of their own")
    c.add_argument("--discover-snvs", action="store_true",
                   help="group the reads by the bases they carry at SNVs found in the reads themselves (GPU with the device front end): a "
                        "position near the locus at which two bases each occur in enough reads; needs --call-alleles and no "
                        "--incorporate-snvs")
    c.add_argument("--snv-discover-window", type=int, default=8192, metavar="N",
                   help="--discover-snvs: how far on either side of the flanked locus SNVs are looked for (1 .. 65536)")
    c.add_argument("--snv-min-base-qual", type=int, default=20)
    c.add_argument("--significant-clip-threshold", type=int, default=100)
    c.add_argument("--use-methyl", "-m", action="store_true",
                   help="5-methyl CpG calls from the reads' MM / ML tags (GPU): m / mc per read, am / amc per called allele")
    c.add_argument("--methyl-threshold", type=int, default=127, help="--use-methyl: a site counts as methylated above this ML value (0 .. 255)")
    c.add_argument("--skip-supplementary", "--skip-supp", dest="skip_supplementary", action="store_true",
                   help="leave out supplementary alignment records (flag 0x800)")
    c.add_argument("--skip-secondary", "--skip-sec", dest="skip_secondary", action="store_true",
                   help="leave out secondary alignment records (flag 0x100)")
    c.add_argument("--unique-reads", action="store_true",
                   help="use a read name once per locus, by its first record that is not skipped (GPU with the device front end); "
                        "with one of these three switches a kept read that has a supplementary and another record over the locus "
                        "is marked chimeric_in_region, and --max-reads caps the records that are left")
    c.add_argument("--gff", "--annotation-file", dest="annotation_file", default=None, metavar="PATH",
                   help="BGZF-compressed GFF3 / GTF file (a GTF when .gtf occurs in PATH) with a PATH.tbi next to it: every locus lists the "
                        "ids of the features it overlaps (annotations in the JSON report, ANNOT in the VCF); each contig's part of the "
                        "file is read once, where --front-end says (GPU or host cores)")
    c.add_argument("--sample-id", default=None)
    c.add_argument("--processes", type=int, default=1)
    c.add_argument("--seed", type=int, default=None)
    c.add_argument("--rc-method", choices=("repalign",), default="repalign")
    c.add_argument("--max-rcn-iters", type=int, default=50)
    c.add_argument("--min-read-align-score", type=float, default=0.1)
    # `strkit mi` (strkit/entry.py: the mi sub-parser) for this project's own call files
    m = sub.add_parser("mi", help="Mendelian inheritance and the de novo test of a child / mother / father trio (GPU)")
    m.add_argument("child_calls", metavar="child-calls")
    m.add_argument("mother_calls", metavar="mother-calls")
    m.add_argument("father_calls", metavar="father-calls")
    m.add_argument("--caller", choices=("strkit-json", "strkit-vcf"), default="strkit-json", help="the format of the three call files")
    m.add_argument("--widen", type=float, default=0.0, help="share of each bound by which the parents' 95 %% intervals grow")
    m.add_argument("--contig", action="append", default=None, help="only this contig (may be given more than once)")
    m.add_argument("--json", default=None, metavar="PATH", help="write the report as JSON (stdout: to standard output)")
    m.add_argument("--no-tsv", action="store_true", help="do not print the table of output loci")
    m.add_argument("--mismatch-out-mi", choices=("strict", "pm1", "ci_95", "ci_99", "seq", "sl", "sl_pm1"), default="pm1",
                   help="without --test: the kind of inheritance whose failures are listed")
    m.add_argument("--hist", action="store_true", help="print the inheritance rates per bin of locus length")
    m.add_argument("--bin-width", type=int, default=10)
    m.add_argument("--test", nargs="?", default="none", const="x2", choices=("none", "x2", "wmw", "wmw-gt"),
                   help="de novo test per locus on the read-level copy numbers (the flag alone: x2)")
    m.add_argument("--sig-level", type=float, default=0.05)
    m.add_argument("--mt-corr", default="none",
                   choices=("none", "bonferroni", "sidak", "holm-sidak", "holm", "simes-hochberg", "fdr_bh", "fdr_by", "fdr_tsbh", "fdr_tsbky"),
                   help="correction for multiple testing (the two-stage methods fdr_tsbh and fdr_tsbky are refused)")
    m.add_argument("--only-phased", action="store_true", help="strkit-vcf: only loci where all three members carry a phase set")
    m.add_argument("--seed", type=int, default=None, help="seeds the split of a one-peak locus's reads into two groups (strkit-json)")
    return ap


def main_mi(ap: argparse.ArgumentParser, a) -> int:
    from . import mi
    if not 0.0 < a.sig_level < 1.0:
        ap.error("--sig-level must be inside (0, 1)")
    if a.widen < 0 or a.bin_width < 1:
        ap.error("--widen must be >= 0 and --bin-width >= 1")
    if a.mt_corr in ("fdr_tsbh", "fdr_tsbky"):
        ap.error(f"--mt-corr {a.mt_corr}: the two-stage methods fdr_tsbh and fdr_tsbky are not supported")
    trio, out, res = mi.run_mi(a.child_calls, a.mother_calls, a.father_calls, caller=a.caller, widen=a.widen, contigs=a.contig,
                               test=a.test, sig_level=a.sig_level, mt_corr=a.mt_corr, mismatch_out_mi=a.mismatch_out_mi,
                               only_phased=a.only_phased, seed=mi.DEFAULT_SEED if a.seed is None else a.seed, bin_width=a.bin_width)
    if res is None:
        return 1
    if not a.no_tsv:
        sys.stdout.write(mi.locus_tsv(trio, out, res))
    sys.stdout.write(mi.summary_text(res, a.widen) + "\n")
    if a.hist:
        sys.stdout.write(mi.histogram_text(res, a.bin_width) + "\n")
    if a.json:
        mi.write_report_json(trio, out, res, a.json)
    return 0


def main(argv=None) -> int:
    ap = build_parser()
    a = ap.parse_args(argv)
    if a.cmd == "mi":
        return main_mi(ap, a)
    if a.consensus and not a.call_alleles:
        ap.error("--consensus needs --call-alleles")
    if a.max_mdn_poa_length < 0:
        ap.error("--max-mdn-poa-length must be >= 0")
    if a.count_kmers in ("peak", "both") and not a.call_alleles:
        ap.error(f"--count-kmers {a.count_kmers} needs --call-alleles")
    if (a.use_hp or a.incorporate_snvs) and not a.call_alleles:
        ap.error("--use-hp / --incorporate-snvs need --call-alleles")
    if a.snv_phase_sets and not a.incorporate_snvs:
        ap.error("--snv-phase-sets needs --incorporate-snvs")
    if a.discover_snvs and not a.call_alleles:
        ap.error("--discover-snvs needs --call-alleles")
    if a.discover_snvs and a.incorporate_snvs:
        ap.error("--discover-snvs and --incorporate-snvs are two sources of candidate SNVs: give one of them")
    if not 1 <= a.snv_discover_window <= 65536:
        ap.error("--snv-discover-window must be in 1 .. 65536")
    if a.ploidy is not None:
        if not a.call_alleles:
            ap.error("--ploidy needs --call-alleles")
        if a.n_alleles != 2:
            ap.error("--ploidy and --n-alleles are two ways to say the same thing: give one of them")
        from .ploidy import load_ploidy_config
        try:
            load_ploidy_config(a.ploidy)
        except ValueError as e:
            ap.error(str(e))
    if not 0 <= a.methyl_threshold <= 255:
        ap.error("--methyl-threshold must be in 0 .. 255")
    import os
    if a.annotation_file and not (os.path.isfile(a.annotation_file) and os.path.isfile(a.annotation_file + ".tbi")):
        ap.error(f"--gff {a.annotation_file}: the file and its tabix index ({a.annotation_file}.tbi) must exist")
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:   # python -m torch.distributed.run --nproc-per-node N -m strkit_amd call ...: one rank per GPU
        from .frontend.gather import SHARDING_REFUSALS
        for name in SHARDING_REFUSALS:      # before the process group is made, in the words of call_sample's refusals
            if getattr(a, name):
                ap.error(SHARDING_REFUSALS[name])
        import torch
        import torch.distributed as dist
        local = int(os.environ.get("LOCAL_RANK", "0"))
        torch.cuda.set_device(local)
        os.environ.setdefault("STRKIT_AMD_DEVICE", str(local))
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    from .frontend import call_sample, write_json
    from .repeat_count_params import RepeatCountParams
    rc = RepeatCountParams("repalign", a.max_rcn_iters, 3, 1)   # params.py:26-27,45
    rep = call_sample(a.read_file, a.ref, a.loci, flank_size=a.flank_size, realign=a.realign,
                      min_avg_phred=a.min_avg_phred, max_reads=a.max_reads, respect_ref=a.respect_ref,
                      sample_id=a.sample_id, processes=a.processes, rc_params=rc,
                      min_read_align_score=a.min_read_align_score, front_end=a.front_end, span_bytes=a.span_mb << 20,
                      count_kmers=a.count_kmers, consensus_method=a.consensus_method, max_mdn_poa_length=a.max_mdn_poa_length,
                      **(dict(use_hp=a.use_hp, snv_vcf=a.incorporate_snvs, snv_min_base_qual=a.snv_min_base_qual,
                              significant_clip_threshold=a.significant_clip_threshold) if a.use_hp or a.incorporate_snvs or a.discover_snvs else {}),
                      **(dict(discover_snvs=True, snv_discover_window=a.snv_discover_window) if a.discover_snvs else {}),
                      **(dict(use_methyl=True, methyl_threshold=a.methyl_threshold) if a.use_methyl else {}),
                      **(dict(ploidy=a.ploidy) if a.ploidy is not None else {}),
                      **(dict(snv_phase_sets=True) if a.snv_phase_sets else {}),
                      **{k: True for k in ("skip_supplementary", "skip_secondary", "unique_reads") if getattr(a, k)},
                      **(dict(annotation_file=a.annotation_file) if a.annotation_file else {}),
                      **(dict(call_alleles=True, consensus=a.consensus or bool(a.vcf), seed=a.seed, n_alleles=a.n_alleles)
                         if a.call_alleles else {}))
    if world > 1:
        import torch.distributed as dist
        rank0 = dist.get_rank() == 0
        dist.destroy_process_group()
        if not rank0:
            return 0
    if a.vcf:
        from .frontend.fasta import Fasta
        from .frontend.output import write_vcf
        write_vcf(rep, a.vcf, Fasta(a.ref), a.sample_id)
    if a.json == "-":
        import json
        json.dump(rep, sys.stdout, indent=1)
    else:
        write_json(rep, a.json)
    return 0


if __name__ == "__main__":
    sys.exit(main())
