"""CPU: the candidate reader of --incorporate-snvs (frontend/snv_vcf.py): plain and gzip input, which records count, contig
names with and without "chr", the order."""
import gzip

import numpy as np
import pytest

from strkit_amd.frontend.bam import _bgzf_blocks
from strkit_amd.frontend.snv_vcf import read_snv_vcf

VCF = """##fileformat=VCFv4.2
##contig=<ID=chr1>
#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO
chr1\t300\trs3\tA\tG\t.\t.\t.
chr1\t100\trs1\tc\tt\t.\t.\t.
chr1\t200\t.\tG\tA,T\t.\t.\t.
chr1\t250\tindel\tGA\tG\t.\t.\t.
chr1\t260\tins\tG\tGA\t.\t.\t.
chr1\t270\tmulti\tG\tA,TT\t.\t.\t.
chr1\t280\tsym\tG\t<DEL>\t.\t.\t.
chr1\t290\tstar\tG\t*\t.\t.\t.
chr1\t295\tnoalt\tG\t.\t.\t.\t.
chr1\t300\tdup\tA\tC\t.\t.\t.
2\t50\trs9\tT\tC\t.\t.\t.
short line
"""


@pytest.mark.parametrize("kind", ["plain", "gzip", "bgzf"])
def test_reads_plain_and_compressed_text_and_keeps_single_base_records(tmp_path, kind):
    path = tmp_path / ("snvs.vcf" if kind == "plain" else "snvs.vcf.gz")
    raw = VCF.encode()
    path.write_bytes(raw if kind == "plain" else gzip.compress(raw) if kind == "gzip" else _bgzf_blocks(raw))
    c = read_snv_vcf(str(path))
    assert sorted(c.by_contig) == ["2", "chr1"]
    one = c.contig("chr1")
    assert one.pos.dtype == np.int64 and one.pos.tolist() == [99, 199, 299]          # 0-based, ascending, one per position
    assert one.ids == ["rs1", "", "rs3"] and one.ref == ["C", "G", "A"]
    assert c.snv_id("chr1", 0) == "rs1" and c.snv_id("chr1", 1) == "chr1_200"


def test_contig_names_with_and_without_the_prefix(tmp_path):
    path = tmp_path / "snvs.vcf"
    path.write_text(VCF)
    c = read_snv_vcf(str(path))
    assert c.contig("1") is c.contig("chr1") and c.contig("chr2") is c.contig("2")
    assert c.contig("chr2").pos.tolist() == [49] and c.contig("chr3") is None and c.contig("3") is None
