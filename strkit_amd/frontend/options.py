"""The options of a `call` run, written once: the dataclass, its checks, the constants of the reference's parameters, and
the `parameters` block of the report."""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass

from .. import _lib
from ..alleles import AlleleParams
from ..batch import MIN_READ_ALIGN_SCORE
from ..phasing import PhaseParams
from ..repeat_count_params import RepeatCountParams
from .extract import MIN_AVG_PHRED

MAX_READS = 250                 # params.max_reads default (strkit/call/params.py:21)
DEFAULT_REF_MAX_ITERS = 250     # call_locus.py:71 default_ref_max_iters (100 there is only the "slow" warning level, :72)
VCF_ANCHOR_SIZE = 5             # params.vcf_anchor_size default
COUNT_KMERS_MODES = ("none", "peak", "read", "both")
CONSENSUS_METHODS = ("best_rep", "poa")


@dataclass
class CallOptions:
    """The knobs of `strkit call` this path honours (strkit/call/params.py:20-50) plus the two semantic switches of the
    read-side counter that the reference's tree does not pin: tools/compare_strkit_json.py sweeps them."""
    flank_size: int = 70
    realign: bool = False
    min_avg_phred: int = MIN_AVG_PHRED
    max_reads: int = MAX_READS
    respect_ref: bool = False
    rc_params: RepeatCountParams | None = None
    min_read_align_score: float = MIN_READ_ALIGN_SCORE
    tie_rule: int = _lib.STRK_TIE_FIRST
    end_flags: int = _lib.STRK_SG_ALL
    narrowing: int = _lib.STRK_NARROW_NONE
    # genotypes (off by default).  `call_alleles`: a genotype per locus (call, intervals,
    # peaks, a peak label `p` per read) from the GPU allele caller, with the locus seed alleles.locus_seed(seed, locus index).
    # `consensus` (needs call_alleles): the sequence of every allele and of its start anchor as peaks.seqs /
    # peaks.start_anchor_seqs.  `seed`: the run seed (an int once a run has started).  `n_alleles`: 1 or 2, for all contigs or
    # per contig in a dict.  Then the caller's parameters and the two limits of strkit/call/params.py:67-68 for the tract
    # groups of long alleles.
    call_alleles: bool = False
    consensus: bool = False
    seed: int | None = None
    n_alleles: int | dict = 2
    allele_params: AlleleParams | None = None
    large_consensus_length: int = 1200
    max_n_large_consensus_reads: int = 20
    # What PoaCallOptions below turns into fields, at the values a CallOptions always has (plain class attributes, not
    # fields: every consumer can read them from either type).
    consensus_method = "best_rep"
    max_mdn_poa_length = 5000
    # motif-sized k-mer counts (strkit/call/params.py count_kmers): "read" = every kept read record gets `kmers`, the counts of
    # the motif-sized windows of its raw tract; "peak" (needs call_alleles) = a called locus gets peaks.kmers, one dict per
    # peak over all reads labelled with it; "both"; "none"
    count_kmers: str = "none"

    def validate(self) -> None:
        """What must hold before a block is called; needs no file and no device."""
        if self.consensus and not self.call_alleles:
            raise ValueError("consensus=True requires call_alleles=True: allele sequences are those of called alleles")
        if self.consensus_method not in CONSENSUS_METHODS:
            raise ValueError(f"consensus_method must be one of {', '.join(CONSENSUS_METHODS)}: got {self.consensus_method!r}")
        if isinstance(self.max_mdn_poa_length, bool) or not isinstance(self.max_mdn_poa_length, int) or self.max_mdn_poa_length < 0:
            raise ValueError(f"max_mdn_poa_length must be an integer >= 0: got {self.max_mdn_poa_length!r}")
        if self.count_kmers not in COUNT_KMERS_MODES:
            raise ValueError(f"count_kmers must be one of {', '.join(COUNT_KMERS_MODES)}: got {self.count_kmers!r}")
        if self.count_kmers in ("peak", "both") and not self.call_alleles:
            raise ValueError(f"count_kmers={self.count_kmers!r} requires call_alleles=True: peak counts are those of called alleles")
        if self.call_alleles and self.seed is None:
            raise ValueError("call_alleles=True needs a run seed (CallOptions.seed); call_sample draws one when none is given")


@dataclass
class PoaCallOptions(CallOptions):
    """CallOptions plus the two options of the consensus stage.  `consensus_method`: how the sequence of an allele whose
    reads differ is made, "best_rep" = one of its reads or "poa" = the consensus of its reads by partial-order
    alignment (§12).  `max_mdn_poa_length`: the median read length above which an allele keeps its best representative under
    "poa" (strkit/call/params.py max_mdn_poa_length).  They live in a type of their own so that the field list of CallOptions,
    which callers and the driver's tests enumerate, stays as it was; call_sample / call_locus take both by name and build this
    type when one of them is given (with_keywords)."""
    consensus_method: str = "best_rep"
    max_mdn_poa_length: int = 5000


POA_OPTION_NAMES = ("consensus_method", "max_mdn_poa_length")


@dataclass
class PhasedCallOptions(PoaCallOptions):
    """PoaCallOptions plus the options of phasing from files.  `use_hp`: reads are grouped by their `HP` / `PS`
    tags where a locus has enough tagged reads (`strkit call --use-hp`).  `snv_vcf`: a VCF of candidate SNVs; reads are
    grouped by the bases they carry at the useful ones (`--incorporate-snvs`).  `snv_min_base_qual`: the quality a base needs
    to count in an SNV call and distance.  `significant_clip_threshold`: the soft clip from which a read's ends are not
    trusted for SNVs (strkit/call/params.py:61).  `phase_params`: the phased call's other parameters.  Both switches need
    call_alleles.  A type of its own for the reason PoaCallOptions gives."""
    use_hp: bool = False
    snv_vcf: str | None = None
    snv_min_base_qual: int = 20
    significant_clip_threshold: int = 100
    phase_params: PhaseParams | None = None

    def validate(self) -> None:
        super().validate()
        if (self.use_hp or self.snv_vcf) and not self.call_alleles:
            raise ValueError("use_hp / snv_vcf require call_alleles=True: they decide how the reads of a call are grouped")
        for name in ("snv_min_base_qual", "significant_clip_threshold"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int) or v < 0 or (name == "snv_min_base_qual" and v > 255):
                raise ValueError(f"{name} must be an integer >= 0 (a base quality: at most 255): got {v!r}")


PHASE_OPTION_NAMES = ("use_hp", "snv_vcf", "snv_min_base_qual", "significant_clip_threshold", "phase_params")


@dataclass
class MethylCallOptions(PhasedCallOptions):
    """PhasedCallOptions plus methylation from MM / ML tags (`strkit call --use-methyl`).  `use_methyl`: every kept
    read record gets `m` and `mc` (the share and the number of its tract's known CpG sites whose 5mC probability is above the
    threshold), a called locus whose every peak has a value gets peaks.am / peaks.amc.  `methyl_threshold`: that threshold on the
    ML scale, 0 .. 255 (127 in the reference's only call).  The switch does not need call_alleles.  A type of its own for the
    reason PoaCallOptions gives."""
    use_methyl: bool = False
    methyl_threshold: int = 127

    def validate(self) -> None:
        super().validate()
        v = self.methyl_threshold
        if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= 255:
            raise ValueError(f"methyl_threshold must be an integer in 0 .. 255 (the scale of ML): got {v!r}")


METHYL_OPTION_NAMES = ("use_methyl", "methyl_threshold")


@dataclass
class PloidyCallOptions(MethylCallOptions):
    """MethylCallOptions plus the ploidy configuration of the sample (`strkit call --ploidy / --sex-chr`; strkit_amd/ploidy.py).
    `ploidy`: the name of a bundled configuration, the path of a JSON file or a dict of its layout.  Every contig is then called
    with its own number of alleles (1 .. alleles.MAX_ALLELES) and loci on a contig that is ignored or has 0 are
    left out of the run.  It replaces `n_alleles`, which must stay at its default.  A type of its own for the reason
    PoaCallOptions gives."""
    ploidy: str | dict | None = None

    def validate(self) -> None:
        super().validate()
        if self.ploidy is not None:
            from ..ploidy import load_ploidy_config
            load_ploidy_config(self.ploidy)
            if self.n_alleles != CallOptions.n_alleles:
                raise ValueError(f"ploidy and n_alleles ({self.n_alleles!r}) are two ways to say the same thing: give one of them")


PLOIDY_OPTION_NAMES = ("ploidy",)


@dataclass
class PhaseSetCallOptions(PloidyCallOptions):
    """PloidyCallOptions plus phase sets across loci for SNV calls (frontend/phase_sets.py).  `snv_phase_sets`: a
    locus called by its SNVs joins the phase set of the loci before it that share a heterozygous site with it (its two peaks
    turned over where their order disagrees), or opens a new one; its row and its reads get `ps`, and the VCF gets the SNVs as
    records of their own.  Needs `snv_vcf`.  A type of its own for the reason PoaCallOptions gives."""
    snv_phase_sets: bool = False

    def validate(self) -> None:
        super().validate()
        if self.snv_phase_sets and not self.snv_vcf:
            raise ValueError("snv_phase_sets=True requires snv_vcf: the phase sets are those of SNV calls")


PHASE_SET_OPTION_NAMES = ("snv_phase_sets",)


@dataclass
class ReadSelectionCallOptions(PhaseSetCallOptions):
    """PhaseSetCallOptions plus which of the records fetched for a locus are used (frontend/select.py).
    `skip_supplementary` / `skip_secondary`: records with flag 0x800 / 0x100 are left out (`strkit call --skip-supplementary /
    --skip-secondary`).  `unique_reads`: a read name is used once per locus, by its first record that is not left out (the
    reference always does this; here it is a switch, off by default, so that every earlier report keeps its bytes).  With one of
    them on, a kept read that has a supplementary and a non-supplementary record over the locus gets `chimeric_in_region`, and
    `max_reads` caps the records that are left, not the records fetched.  A type of its own for the reason PoaCallOptions gives."""
    skip_supplementary: bool = False
    skip_secondary: bool = False
    unique_reads: bool = False

    def validate(self) -> None:
        super().validate()
        for name in READ_SELECTION_OPTION_NAMES:
            if not isinstance(getattr(self, name), bool):
                raise ValueError(f"{name} must be True or False: got {getattr(self, name)!r}")


READ_SELECTION_OPTION_NAMES = ("skip_supplementary", "skip_secondary", "unique_reads")


@dataclass
class AnnotationCallOptions(ReadSelectionCallOptions):
    """ReadSelectionCallOptions plus locus annotations (frontend/annotations.py; `strkit call --gff /
    --annotation-file`).  `annotation_file`: a BGZF-compressed, tabix-indexed GFF3 or GTF file (a GTF when ".gtf" occurs in the
    path); every row of the report then lists, as `annotations`, the ids of the features its locus overlaps, and the VCF carries
    them as ANNOT.  A type of its own for the reason PoaCallOptions gives."""
    annotation_file: str | None = None

    def validate(self) -> None:
        super().validate()
        if self.annotation_file is not None:
            import os
            if not isinstance(self.annotation_file, str) or not os.path.isfile(self.annotation_file):
                raise ValueError(f"annotation_file {self.annotation_file!r} does not exist")
            if not os.path.isfile(self.annotation_file + ".tbi"):
                raise ValueError(f"annotation_file {self.annotation_file!r} has no tabix index next to it ({self.annotation_file}.tbi): "
                                 f"bgzip the sorted file and run `tabix -p gff` on it")


ANNOTATION_OPTION_NAMES = ("annotation_file",)


@dataclass
class SnvDiscoveryCallOptions(AnnotationCallOptions):
    """AnnotationCallOptions plus candidate SNVs from the reads themselves (frontend/snv_discovery.py; `strkit call
    --discover-snvs`).  `discover_snvs`: reads are grouped by the bases they carry at the useful SNVs, as with `snv_vcf`, and the
    candidate positions come from a pileup of each locus's kept reads instead of a file: a position within `snv_discover_window`
    bases of the flanked locus at which two bases each occur in enough reads.  `snv_min_base_qual` and
    `significant_clip_threshold` apply as they do with a file.  Needs call_alleles; a run has one source of candidates, so it is
    refused together with `snv_vcf` (and `snv_phase_sets` keeps needing `snv_vcf`).  A type of its own for the reason
    PoaCallOptions gives."""
    discover_snvs: bool = False
    snv_discover_window: int = 8192      # a default of the option, not a measured threshold: about half a 15 kb read

    def validate(self) -> None:
        super().validate()
        if not isinstance(self.discover_snvs, bool):
            raise ValueError(f"discover_snvs must be True or False: got {self.discover_snvs!r}")
        w = self.snv_discover_window
        if isinstance(w, bool) or not isinstance(w, int) or not 1 <= w <= 65536:
            raise ValueError(f"snv_discover_window must be an integer in 1 .. 65536: got {w!r}")
        if self.discover_snvs and not self.call_alleles:
            raise ValueError("discover_snvs=True requires call_alleles=True: the SNVs decide how the reads of a call are grouped")
        if self.discover_snvs and self.snv_vcf:
            raise ValueError("discover_snvs=True and snv_vcf are two sources of candidate SNVs: give one of them")


SNV_DISCOVERY_OPTION_NAMES = ("discover_snvs", "snv_discover_window")


def allele_counts(opts):
    """What genotype.n_alleles_of takes for a run: its ploidy configuration where one is set, else its n_alleles."""
    ploidy = getattr(opts, "ploidy", None)
    if ploidy is None:
        return opts.n_alleles
    from ..ploidy import load_ploidy_config
    return load_ploidy_config(ploidy)


def phased(opts) -> bool:
    """Whether a switch of PhasedCallOptions is on (any options type may be asked)."""
    return bool(getattr(opts, "use_hp", False) or getattr(opts, "snv_vcf", None) or getattr(opts, "discover_snvs", False))


def with_keywords(opts: CallOptions | None, **option_keywords) -> CallOptions:
    """`opts` (or the defaults) with the options given by name replaced: dataclasses.replace, after widening a plain
    CallOptions to PoaCallOptions when one of POA_OPTION_NAMES is among them, to PhasedCallOptions for PHASE_OPTION_NAMES, to
    MethylCallOptions for METHYL_OPTION_NAMES, to PloidyCallOptions for PLOIDY_OPTION_NAMES, to PhaseSetCallOptions for
    PHASE_SET_OPTION_NAMES, to ReadSelectionCallOptions for READ_SELECTION_OPTION_NAMES, to AnnotationCallOptions for
    ANNOTATION_OPTION_NAMES, and to SnvDiscoveryCallOptions for SNV_DISCOVERY_OPTION_NAMES.  An unknown name is a TypeError."""
    opts = opts or CallOptions()
    if not isinstance(opts, SnvDiscoveryCallOptions) and any(k in option_keywords for k in SNV_DISCOVERY_OPTION_NAMES):
        opts = SnvDiscoveryCallOptions(**{f.name: getattr(opts, f.name) for f in dataclasses.fields(opts)})
    if not isinstance(opts, AnnotationCallOptions) and any(k in option_keywords for k in ANNOTATION_OPTION_NAMES):
        opts = AnnotationCallOptions(**{f.name: getattr(opts, f.name) for f in dataclasses.fields(opts)})
    if not isinstance(opts, ReadSelectionCallOptions) and any(k in option_keywords for k in READ_SELECTION_OPTION_NAMES):
        opts = ReadSelectionCallOptions(**{f.name: getattr(opts, f.name) for f in dataclasses.fields(opts)})
    if not isinstance(opts, PhaseSetCallOptions) and any(k in option_keywords for k in PHASE_SET_OPTION_NAMES):
        opts = PhaseSetCallOptions(**{f.name: getattr(opts, f.name) for f in dataclasses.fields(opts)})
    if not isinstance(opts, PloidyCallOptions) and any(k in option_keywords for k in PLOIDY_OPTION_NAMES):
        opts = PloidyCallOptions(**{f.name: getattr(opts, f.name) for f in dataclasses.fields(opts)})
    if not isinstance(opts, MethylCallOptions) and any(k in option_keywords for k in METHYL_OPTION_NAMES):
        opts = MethylCallOptions(**{f.name: getattr(opts, f.name) for f in dataclasses.fields(opts)})
    if not isinstance(opts, PhasedCallOptions) and any(k in option_keywords for k in PHASE_OPTION_NAMES):
        opts = PhasedCallOptions(**{f.name: getattr(opts, f.name) for f in dataclasses.fields(opts)})
    if not isinstance(opts, PoaCallOptions) and any(k in option_keywords for k in POA_OPTION_NAMES):
        opts = PoaCallOptions(**{f.name: getattr(opts, f.name) for f in dataclasses.fields(opts)})
    return dataclasses.replace(opts, **option_keywords)


def report_parameters(opts: CallOptions, processes: int) -> dict:
    """The `parameters` block of the report: the always-present keys, then those of every switch that is not at its default."""
    ap = opts.allele_params or AlleleParams()
    return {"flank_size": opts.flank_size, "realign": opts.realign, "min_avg_phred": opts.min_avg_phred,
            "max_reads": opts.max_reads, "respect_ref": opts.respect_ref, "rc_method": "repalign",
            "min_read_align_score": opts.min_read_align_score, "processes": processes,
            **({"tie_rule": opts.tie_rule} if opts.tie_rule != _lib.STRK_TIE_FIRST else {}),
            **({"end_flags": opts.end_flags} if opts.end_flags != _lib.STRK_SG_ALL else {}),
            **({"narrowing": opts.narrowing} if opts.narrowing != _lib.STRK_NARROW_NONE else {}),
            **({"call_alleles": True, "seed": opts.seed, "n_alleles": opts.n_alleles, "min_reads": ap.min_reads,
                "min_allele_reads": ap.min_allele_reads, "num_bootstrap": ap.num_bootstrap} if opts.call_alleles else {}),
            **({"consensus": True, "large_consensus_length": opts.large_consensus_length,
                "max_n_large_consensus_reads": opts.max_n_large_consensus_reads} if opts.consensus else {}),
            **({"consensus_method": opts.consensus_method} if opts.consensus_method != "best_rep" else {}),
            **({"max_mdn_poa_length": opts.max_mdn_poa_length} if opts.max_mdn_poa_length != 5000 else {}),
            **({"count_kmers": opts.count_kmers} if opts.count_kmers != "none" else {}),
            **({"use_hp": True} if getattr(opts, "use_hp", False) else {}),
            **({"snv_vcf": opts.snv_vcf, "snv_min_base_qual": opts.snv_min_base_qual} if getattr(opts, "snv_vcf", None) else {}),
            **({"significant_clip_threshold": opts.significant_clip_threshold} if phased(opts) else {}),
            **({"use_methyl": True} if getattr(opts, "use_methyl", False) else {}),
            **({"methyl_threshold": opts.methyl_threshold} if getattr(opts, "use_methyl", False) and opts.methyl_threshold != 127 else {}),
            **({"ploidy": opts.ploidy} if getattr(opts, "ploidy", None) is not None else {}),
            **({"snv_phase_sets": True} if getattr(opts, "snv_phase_sets", False) else {}),
            **{name: True for name in READ_SELECTION_OPTION_NAMES if getattr(opts, name, False)},
            **({"annotation_file": opts.annotation_file} if getattr(opts, "annotation_file", None) else {}),
            **({"discover_snvs": True, "snv_discover_window": opts.snv_discover_window, "snv_min_base_qual": opts.snv_min_base_qual}
               if getattr(opts, "discover_snvs", False) else {})}
