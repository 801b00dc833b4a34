"""The environment variables libhuygens_hip.so reads are exactly those INTEGRATION.md section 6
lists: every string literal passed to getenv under huygens_amd/csrc/ against the table's first
column.  A settled A/B switch that stays behind, or a new one nobody recorded, fails here."""
import pathlib
import re

ROOT = pathlib.Path(__file__).resolve().parent.parent


def test_getenv_names_match_integration_table():
    read, calls, literal_calls = set(), 0, 0
    for src in sorted((ROOT / "huygens_amd" / "csrc").iterdir()):
        if src.suffix not in (".hip", ".h"):
            continue
        text = src.read_text()
        names = re.findall(r'\bgetenv\s*\(\s*"([^"]+)"\s*\)', text)
        calls += len(re.findall(r"\bgetenv\s*\(", text))
        literal_calls += len(names)
        read |= set(names)
    assert read, "no getenv call found under huygens_amd/csrc"
    # (a computed name would escape the comparison below)
    assert calls == literal_calls, "a getenv call under huygens_amd/csrc does not name its variable as a literal"

    doc = (ROOT / "INTEGRATION.md").read_text()
    section = doc.split("## 6. Environment variables", 1)[1].split("\n## ", 1)[0]
    listed = set(re.findall(r"^\|\s*`(HZ_[A-Z0-9_]+)`\s*\|", section, flags=re.M))
    assert listed, "INTEGRATION.md section 6 lists no variable"
    assert read == listed, (f"read by the library but not listed: {sorted(read - listed)}; "
                            f"listed but not read: {sorted(listed - read)}")
