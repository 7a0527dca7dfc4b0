"""The library's one source list (seastar_amd/build.py): every source under
csrc is built, and every header the build reads makes a built library stale."""
import glob
import os

from seastar_amd import build

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "seastar_amd", "csrc")


def test_sources_and_headers_cover_csrc():
    on_disk = {p for ext in ("*.hip", "*.cc") for p in glob.glob(os.path.join(CSRC, ext))}
    # checksummer_packet.cc needs the reference's packet type: built by its own test only
    on_disk.discard(os.path.join(CSRC, "checksummer_packet.cc"))
    assert on_disk and on_disk == set(build.SOURCES)
    stale = set(build.headers())
    csrc_headers = set(glob.glob(os.path.join(CSRC, "*.h")))
    assert csrc_headers and csrc_headers <= stale
    assert {os.path.join(build.REPO_DIR, "include", h) for h in ("sccsum.h", "sccsum_diag.h")} <= stale
