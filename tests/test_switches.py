"""The product reads exactly three RV_* environment variables (DESIGN.md,
"Switches"): RV_CONV_DEBUG (a log), RV_SORT_FUSED (the open SORT comparison)
and RV_LIB_VARIANT (the A/B library selector).  Everything else is a handle
option or an argument, so a test can reach both sides.  An experiment that
needs a new switch adds its name here on purpose.

CPU-only: the sources are scanned as text.
"""
import glob
import os
import re

from conftest import REPO

PKG = os.path.join(REPO, "road-vision-system_amd")
ALLOWED = {"RV_CONV_DEBUG", "RV_SORT_FUSED", "RV_LIB_VARIANT"}

GETENV = re.compile(r"""getenv\(\s*"(RV_\w+)"\s*\)""")
ENVIRON = re.compile(r"""(?:environ(?:\.get|\.pop|\.setdefault)?\s*[\[(]|getenv\s*\()\s*["'](RV_\w+)["']""")


def _scan(paths, pattern):
    found = []
    for path in sorted(paths):
        with open(path, encoding="utf-8", errors="replace") as f:
            for no, line in enumerate(f, 1):
                for name in pattern.findall(line):
                    found.append((name, f"{os.path.relpath(path, REPO)}:{no}"))
    return found


def test_environment_switches_are_the_documented_three():
    csrc = [p for ext in ("hip", "h", "c")
            for p in glob.glob(os.path.join(PKG, "csrc", "*." + ext))]
    py = glob.glob(os.path.join(PKG, "rvs_amd", "**", "*.py"), recursive=True)
    assert csrc and py
    found = _scan(csrc, GETENV) + _scan(py, ENVIRON)
    extra = [f"{name} at {where}" for name, where in found if name not in ALLOWED]
    assert not extra, "undocumented environment switches: " + ", ".join(extra)
    missing = ALLOWED - {name for name, _ in found}
    assert not missing, f"documented switches no longer read: {sorted(missing)}"
