"""Fixtures of the segment-guess tests (tests/test_long_guess_emulation.py, the
CPU model; tests/test_gpu_long_guess.py, the kernels): patterns whose DFA has
more than 256 states (the filter stepper) and long lines that the scan parks
at 4 KiB lane chunks (every line of 9 KiB or more is still open 8 KiB past
its owner's chunk start), with short log lines between them. Everything is
generated from fixed seeds.

A parked line is cut into 16,384-byte segments from its start. The runtime's
cut is max(16 KiB, parked bytes / about 260,000 lanes), so it is exactly
16 KiB for any total under about 4 GiB; every case here parks under 2 MiB."""
import collections
import random

SEG = 16384

Case = collections.namedtuple("Case", "name nkw tail alphabet mod expect")
# expect: "zero" -- every walked segment's true entry state is among its
# guesses; "some" -- the case is there to reach the fix kernel's serial re-run;
# None -- no requirement on the miss count

MOD5 = b"^([^k]*k[^k]*k[^k]*k[^k]*k[^k]*k)*[^k]*$"
CASES = [
    Case("kw100", 100, b"", "words", 0, "zero"),
    Case("kw100_mod2", 100, b"", "words", 2, "zero"),
    Case("kw100_mod3", 100, b"", "words", 3, None),
    Case("kw100_mod5", 100, b"", "words", 5, "some"),
    Case("kw100_mod7", 100, b"", "words", 7, "some"),
    Case("kw300_mod3", 300, b"", "words", 3, "some"),
    Case("kw300_mod5", 300, b"", "words", 5, "some"),
    # above 65,535 states: u32 table entries (the <uint32_t> kernels)
    Case("u32_window", 0, b"a[ab]{16}$", "abkx", 0, "zero"),
    Case("u32_mod5", 0, b"a[ab]{13}$|" + MOD5, "abkx", 5, "some"),
]


def pattern_of(case):
    """Keyword cases: (?i) alternation of the first nkw seeded config-4
    keywords, OR (mod > 0) "the number of k in the line is divisible by mod".
    Built on demand: the keywords come from the library, which a GPU test
    module must not load while it is being collected."""
    if not case.nkw:
        return case.tail
    import dgrep

    p = b"(?i)(" + b"|".join(dgrep.synth_keywords(4, case.nkw)) + b")"
    if case.mod:
        p += b"|^(" + b"[^k]*k" * case.mod + b")*[^k]*$"
    return p


CASE_IDS = [c.name for c in CASES]

WORDS = [b"request", b"user", b"cache", b"latency", b"retry", b"shard", b"value", b"node", b"kind", b"yes", b"zone",
         b"token", b"ok"]
# 16384 j and 16384 j +- 1 (j = 1..3; 16384 + 1 leaves a 1-byte last segment)
EDGE_LENGTHS = [SEG - 1, SEG, SEG + 1, 2 * SEG - 1, 2 * SEG, 2 * SEG + 1, 3 * SEG - 1, 3 * SEG, 3 * SEG + 1]


def _body(rnd, alphabet, n):
    if alphabet == "words":
        out = bytearray()
        while len(out) < n:
            out += rnd.choice(WORDS) + b" "
        return out[:n]
    return bytearray(rnd.choices(b"abkx", weights=(46, 46, 3, 5), k=n))


def _set_k_count(rnd, body, mod, residue):
    """Turns k into x until the k count is residue mod `mod`."""
    if not mod:
        return
    while body.count(b"k") % mod != residue:
        q = rnd.randrange(len(body))
        if body[q] == ord("k"):
            body[q] = ord("x")


def _set_tail(body, alphabet, match):
    """abkx lines: the last 17 bytes decide a[ab]{16}$ (14: a[ab]{13}$); a
    line that ends in x matches neither."""
    if alphabet == "abkx":
        body[-17:] = b"abbabaabbbababaab" if match else b"abbabaabbbababaax"


def long_lines(case):
    """The case's long lines (no '\\n' inside), in order; the last one is the
    split's unterminated last line."""
    import dgrep

    rnd = random.Random("long-guess " + case.name)
    kws = dgrep.synth_keywords(4, 100)
    lines = []

    def add(n, match, plant_at=None):
        body = _body(rnd, case.alphabet, n)
        # k-count branch: residue 0 matches; the window / keyword patterns decide by the tail / the plant
        _set_tail(body, case.alphabet, match and not case.mod)
        _set_k_count(rnd, body, case.mod, 0 if match else 1 + rnd.randrange(max(case.mod - 1, 1)))
        if plant_at is not None and case.alphabet == "words":
            kw = bytearray(rnd.choice(kws))
            for i in range(len(kw)):
                if rnd.random() < 0.5:
                    kw[i] -= 32  # (?i)
            body[plant_at:plant_at + len(kw)] = kw
        assert len(body) == n and b"\n" not in body
        lines.append(bytes(body))

    for i in range(4):  # random text, both verdicts
        match = i % 2 == 0
        n = rnd.randrange(30 << 10, 130 << 10)
        add(n, match, plant_at=rnd.randrange(n - 16) if match and not case.mod else None)
    for i, n in enumerate(EDGE_LENGTHS):
        add(n, i % 3 == 0, plant_at=n - 12 if i % 3 == 0 and not case.mod else None)
    add(10000, True, plant_at=5000 if not case.mod else None)  # parked, one segment
    add(60 << 10, True, plant_at=1000)  # MATCHED inside the first segment: a walk of one segment
    add(50 << 10, False, plant_at=SEG - 4)  # a keyword across the first segment edge
    add(2 * SEG + 8, True)  # abkx: the deciding window lies across the last segment edge
    add(70 << 10, False)  # the unterminated last line
    return lines


def split_of(lines):
    """(data, [(start, length)]): the long lines with short log lines between them."""
    rnd = random.Random(len(lines))
    out = bytearray()
    spans = []
    for i, line in enumerate(lines):
        for _ in range(rnd.randrange(1, 6)):
            out += b"2024-05-%02d 12:00:%02d INFO request %d served by node-%d\n" % (
                1 + i % 28, rnd.randrange(60), rnd.randrange(10 ** 6), rnd.randrange(64))
        spans.append((len(out), len(line)))
        out += line
        if i + 1 < len(lines):
            out += b"\n"
    return bytes(out), spans
