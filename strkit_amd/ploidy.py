"""Ploidy configurations: how many alleles a contig has, or that it is left out of a run (`strkit call --ploidy / --sex-chr`,
strkit/ploidy.py, strkit/call/loci.py:224-230).

A configuration is a default count, overrides per contig pattern and ignored contig patterns.  `PloidyConfig.n_of(contig)`
tries the overrides first, in the order given, then the ignored patterns (-> None), else answers the default; patterns are
regular expressions matched with re.fullmatch.  A contig whose answer is None or 0 is not genotyped.  The bundled
configurations are this module's own table (tests/test_ploidy.py holds it equal to the reference's files, kept as
fixtures)."""
from __future__ import annotations

import json
import os
import re
from dataclasses import dataclass, field

from .alleles import MAX_ALLELES

__all__ = ["BUNDLED_PLOIDY_CONFIGS", "MAX_ALLELES", "PloidyConfig", "load_ploidy_config"]

_DIPLOID_XX = {"default": 2, "overrides": {"(chr)?Y": 0, "(chr)?M": 1}}
_DIPLOID_XY = {"default": 2, "overrides": {"(chr)?X": 1, "(chr)?Y": 1, "(chr)?M": 1}}
BUNDLED_PLOIDY_CONFIGS: dict[str, dict] = {
    "haploid": {"default": 1},
    "diploid_autosomes": {"default": 2, "ignore": ["chr(X|Y)"], "overrides": {"(chr)?M": 1}},
    "diploid_xx": _DIPLOID_XX,
    "XX": _DIPLOID_XX,
    "diploid_xy": _DIPLOID_XY,
    "XY": _DIPLOID_XY,
}
_KEYS = {"default", "overrides", "ignore"}


def _count(value, what: str) -> int:
    if isinstance(value, bool) or not isinstance(value, int) or not 0 <= value <= MAX_ALLELES:
        raise ValueError(f"ploidy configuration: {what} must be an integer in 0 .. {MAX_ALLELES}: got {value!r}")
    return value


def _pattern(text, what: str) -> str:
    if not isinstance(text, str):
        raise ValueError(f"ploidy configuration: {what} must be a string (a regular expression): got {text!r}")
    try:
        re.compile(text)
    except re.error as e:
        raise ValueError(f"ploidy configuration: {what} {text!r} is not a regular expression: {e}") from None
    return text


@dataclass(frozen=True)
class PloidyConfig:
    default: int
    overrides: dict = field(default_factory=dict)    # pattern -> count, tried in this order
    ignore: tuple = ()                               # patterns of contigs that are left out

    def __post_init__(self):
        _count(self.default, "default")
        if not isinstance(self.overrides, dict):
            raise ValueError(f"ploidy configuration: overrides must map patterns to counts: got {self.overrides!r}")
        for k, v in self.overrides.items():
            _pattern(k, "the override pattern")
            _count(v, f"the override of {k!r}")
        if isinstance(self.ignore, (str, bytes)) or not isinstance(self.ignore, (list, tuple, set, frozenset)):
            raise ValueError(f"ploidy configuration: ignore must be a list of patterns: got {self.ignore!r}")
        object.__setattr__(self, "ignore", tuple(_pattern(k, "the ignored pattern") for k in self.ignore))

    def n_of(self, contig: str) -> int | None:
        """The number of alleles of a contig; None for one that is ignored."""
        for k, v in self.overrides.items():
            if re.fullmatch(k, contig):
                return v
        for k in self.ignore:
            if re.fullmatch(k, contig):
                return None
        return self.default

    def called(self, contig: str) -> bool:
        """Whether loci on this contig are genotyped (strkit/call/loci.py:224-230: neither ignored nor without a copy)."""
        return bool(self.n_of(contig))

    def to_dict(self) -> dict:
        return {"default": self.default, **({"overrides": dict(self.overrides)} if self.overrides else {}),
                **({"ignore": list(self.ignore)} if self.ignore else {})}


def load_ploidy_config(id_or_path) -> PloidyConfig:
    """A configuration from the name of a bundled one, the path of a JSON file, a dict of the file's layout, or a PloidyConfig
    itself.  The keys must be `default` (required), `overrides` and `ignore`; anything else is a ValueError."""
    if isinstance(id_or_path, PloidyConfig):
        return id_or_path
    if isinstance(id_or_path, dict):
        d, src = id_or_path, "the dict given"
    elif isinstance(id_or_path, str) and id_or_path in BUNDLED_PLOIDY_CONFIGS:
        d, src = BUNDLED_PLOIDY_CONFIGS[id_or_path], id_or_path
    else:
        src = os.fspath(id_or_path)
        try:
            with open(src) as fh:
                d = json.load(fh)
        except FileNotFoundError:
            raise ValueError(f"ploidy configuration {src!r}: neither a bundled name ({', '.join(BUNDLED_PLOIDY_CONFIGS)}) "
                             f"nor a file") from None
        except json.JSONDecodeError as e:
            raise ValueError(f"ploidy configuration {src!r}: not JSON: {e}") from None
    if not isinstance(d, dict) or "default" not in d or not set(d) <= _KEYS:
        raise ValueError(f"ploidy configuration ({src}): the keys must be default, and optionally overrides and ignore: got "
                         f"{sorted(d) if isinstance(d, dict) else d!r}")
    return PloidyConfig(d["default"], d.get("overrides", {}), d.get("ignore", ()))
