# The sample span of csrc/augment.hip under the LDS bank model of ds_read_b32 (two groups of 32 lanes, bank = word mod 32,
# cycles per group = the most distinct addresses on one bank): the Hankel operand "frame li, sample c" = span[li * stride + c]
# with one pad word after every 2^a samples (stride = 2^a m, m odd, a >= 2) against the unpadded layout.
def pad_shift(stride):
    a = 0
    while not (stride >> a) & 1:
        a += 1
    return a if a >= 2 else 31


def cycles(stride, padded=True):
    sh = pad_shift(stride) if padded else 31
    worst = total = n = 0
    for c in range(64):
        for hi in (0, 1):
            banks = {}
            for li in range(32):
                s = li * stride + hi * 4 + c
                addr = s + (s >> sh)
                banks.setdefault(addr % 32, set()).add(addr)
            w = max(len(v) for v in banks.values())
            worst, total, n = max(worst, w), total + w, n + 1
    return total / n, worst


if __name__ == "__main__":
    for name, stride in (("response (Toeplitz)", 32), ("22050 -> 16000", 441), ("1 -> 2", 1), ("2 -> 1", 2), ("22050 -> 24000", 147),
                         ("24000 -> 22050", 160), ("48000 -> 22050", 320)):
        (pm, pw), (um, uw) = cycles(stride), cycles(stride, False)
        print(f"{name:22s} stride {stride:4d} pad shift {pad_shift(stride):2d}: padded mean {pm:.2f} worst {pw}, unpadded mean {um:.2f} worst {uw}")
