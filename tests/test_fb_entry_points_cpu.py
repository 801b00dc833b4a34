"""Every extern "C" hz_fb_* function under huygens_amd/csrc/ holds what the table above
hz_fbi::Entry in hz_fb_impl.h says it holds: SampleLock (the sample path), HandleLock or Entry (the
guarded calls) taken before the body's first use of `h->`, or nothing -- and then its name stands
in LOCK_FREE below, which must equal the table's list.  A new entry point nobody classified, or one
that touches the handle ahead of its guard, fails here."""
import pathlib
import re

CSRC = pathlib.Path(__file__).resolve().parent.parent / "huygens_amd" / "csrc"

LOCK_FREE = {
    "hz_fb_info", "hz_fb_state_size", "hz_fb_get_stream", "hz_fb_tune", "hz_fb_set_target_groups",
    "hz_fb_set_path", "hz_fb_last_path", "hz_fb_lti_last_chunk", "hz_fb_lti_plan", "hz_fb_tune_lti",
    "hz_fb_tune_stream", "hz_fb_stream_info", "hz_fb_set_time_shard_fill", "hz_fb_tune_response_engine",
    "hz_fb_tune_modal", "hz_fb_modal_info", "hz_fb_response_engine", "hz_fb_tune_response",
    "hz_fb_time_shard_info", "hz_fb_response_info",
}
LIFECYCLE = {"hz_fb_create_shard", "hz_fb_create", "hz_fb_destroy"}   # no other thread has the handle

GUARDS = {
    "sample": re.compile(r"\bhz_fbi::SampleLock\b\s*\w*\(h\)"),
    "handle": re.compile(r"\bhz_fbi::HandleLock \w+\(h\);"),
    "entry": re.compile(r"\bhz_fbi::Entry \w+\(h, \"(\w+)\"(, false)?\);\s*HZ_TRY\(\w+\.status\);"),
}


def definitions():
    """name -> body of every `int hz_fb_*(...) {` at the start of a line"""
    found = {}
    for src in sorted(CSRC.iterdir()):
        if src.suffix not in (".hip", ".h"):
            continue
        text = src.read_text()
        for m in re.finditer(r"^int (hz_fb_\w+)\([^;{]*\)\s*\{", text, flags=re.M):
            depth, i = 1, m.end()
            while depth:
                depth += {"{": 1, "}": -1}.get(text[i], 0)
                i += 1
            assert m.group(1) not in found, m.group(1)
            found[m.group(1)] = re.sub(r"//[^\n]*", "", text[m.end():i])
    return found


def table():
    """class -> names, from the comment table in hz_fb_impl.h (`*`: Entry with state_back false)"""
    text = (CSRC / "hz_fb_impl.h").read_text()
    body = text.split("//   sample path", 1)[1].split("// Entry:", 1)[0]
    heads = [("sample", "(SampleLock):"), ("handle", "//   guarded, host staging only"),
             ("entry", "//   guarded, device work"), ("lock_free", "//   lock-free:"), ("lifecycle", "//   lifecycle")]
    cut = [0] + [body.index(mark) for _, mark in heads[1:]] + [len(body)]
    return {name: set(re.findall(r"\bhz_fb_\w+\*?", body[cut[i]:cut[i + 1]])) for i, (name, _) in enumerate(heads)}


def test_every_entry_point_is_classified_and_guarded_as_the_table_says():
    defs, tab = definitions(), table()
    assert len(defs) > 50, sorted(defs)
    assert tab["lock_free"] == LOCK_FREE, sorted(tab["lock_free"] ^ LOCK_FREE)
    assert tab["lifecycle"] == LIFECYCLE, sorted(tab["lifecycle"] ^ LIFECYCLE)
    listed = [n.rstrip("*") for names in tab.values() for n in names]
    assert len(listed) == len(set(listed)), "a function stands in two classes of the table"
    assert set(listed) == set(defs), (f"defined but not in the table: {sorted(set(defs) - set(listed))}; "
                                      f"in the table but not defined: {sorted(set(listed) - set(defs))}")
    for name, body in sorted(defs.items()):
        if name in LIFECYCLE:
            continue
        held = {kind: rx.search(body) for kind, rx in GUARDS.items()}
        kinds = [k for k, m in held.items() if m]
        if name in LOCK_FREE:
            assert not kinds, f"{name} is listed lock-free but takes {kinds}"
            continue
        want = next(k for k in ("sample", "handle", "entry") if name in {n.rstrip("*") for n in tab[k]})
        assert kinds == [want], f"{name}: the table says {want}, the body takes {kinds or 'nothing'}"
        use = re.search(r"\bh->", body)
        assert not use or held[want].start() < use.start(), f"{name} uses h-> before it takes its guard"
        if want == "entry":
            assert held[want].group(1) == name, f"{name} names itself {held[want].group(1)} in its Entry"
            assert (held[want].group(2) is not None) == (name + "*" in tab["entry"]), \
                f"{name}: state_back in the code and the table's * differ"
