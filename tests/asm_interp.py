"""Integer interpreter for the inline-assembly blocks of csrc/mont_asm.h (test helper, no GPU).

parse_header() reads every `#define HK_<KIND>_ASM_<FIELD>` of the header SOURCE TEXT: the instruction list, the
constraint lists that bind the %k operands, the `u32 t0 = a.v[0], ...` initialisers and the `r.v[i] = ti;` stores.
Block.compile() turns the straight-line instruction list into one Python function on integers.  Because the blocks
have no branches, two properties are checked exactly while compiling, before any operand is run:
  * every register that is read has been written before (or bound to an initialised operand) - the way a tied
    operand form goes wrong;
  * every physical register (vN, sN, vcc) the block writes is in its clobber list, and every output operand is
    early-clobber (&), so the compiler may not overlap it with an input that is still to be read.
An unknown mnemonic or operand form raises AsmError: a new instruction in the generator has to be taught here.
The compiled function also records, per VCC-consuming instruction, which VCC states it saw (carry coverage).
"""
import re

M32 = 0xFFFFFFFF
VCC_CONSUMERS = ("v_addc_co_u32", "v_subb_co_u32", "v_cndmask_b32")


class AsmError(Exception):
    pass


class Block:
    def __init__(self, kind, field, params, instrs, outs, ins, clobbers, inits, stores):
        self.kind, self.field, self.params = kind, field, params
        self.instrs = instrs            # ["v_add_co_u32 %0, vcc, %0, %8", ...]
        self.outs = outs                # [(constraint, c variable)]
        self.ins = ins                  # [(constraint, c expression)]
        self.clobbers = clobbers
        self.inits = inits              # c variable -> c expression (or None when declared without initialiser)
        self.stores = stores            # [(limb index of r, c variable)]

    def vcc_consumers(self):
        return [i for i, ins in enumerate(self.instrs) if ins.split()[0] in VCC_CONSUMERS]

    # ---- compilation to Python ----------------------------------------------------------------------------
    def compile(self):
        """-> fn(a_limbs, b_limbs, cov) -> result limbs; cov[i] |= 1 << vcc for every VCC consumer i."""
        defined = set()
        written_phys = set()
        src = ["def _blk(a, b, cov):"]

        def cexpr(e):
            m = re.fullmatch(r"([ab])\.v\[(\d+)\]", e)
            if not m:
                raise AsmError("%s: operand expression %r" % (self.name(), e))
            if m.group(1) not in self.params:
                raise AsmError("%s: %r is not a macro parameter" % (self.name(), e))
            return "%s[%s]" % (m.group(1), m.group(2))

        nout = len(self.outs)
        for k, (con, var) in enumerate(self.outs):
            if "&" not in con:
                raise AsmError("%s: output operand %%%d (%s) is not early-clobber" % (self.name(), k, con))
            if con.startswith("+"):
                if self.inits.get(var) is None:
                    raise AsmError("%s: read-write operand %%%d (%s) has no initialiser" % (self.name(), k, var))
                src.append("    o%d = %s" % (k, cexpr(self.inits[var])))
                defined.add("o%d" % k)
            elif not con.startswith("="):
                raise AsmError("%s: output constraint %r" % (self.name(), con))
        for k, (con, e) in enumerate(self.ins):
            if con != "v":
                raise AsmError("%s: input constraint %r" % (self.name(), con))
            src.append("    o%d = %s" % (nout + k, cexpr(e)))
            defined.add("o%d" % (nout + k))
        nops = nout + len(self.ins)

        def reg(tok, write=False):
            """python variable of a 32-bit register token"""
            m = re.fullmatch(r"%(\d+)", tok)
            if m:
                k = int(m.group(1))
                if k >= nops:
                    raise AsmError("%s: operand %s does not exist" % (self.name(), tok))
                if write and k >= nout:
                    raise AsmError("%s: writes input operand %s" % (self.name(), tok))
                name = "o%d" % k
            elif re.fullmatch(r"[vs]\d+", tok):
                name = tok
                if write:
                    written_phys.add(tok)
            else:
                raise AsmError("%s: register %r" % (self.name(), tok))
            if write:
                defined.add(name)
            elif name not in defined:
                raise AsmError("%s: %s is read before it is written" % (self.name(), tok))
            return name

        def val(tok):
            if re.fullmatch(r"0x[0-9a-fA-F]{1,8}", tok):
                return str(int(tok, 16))
            if re.fullmatch(r"-?\d+", tok):
                return str(int(tok) & M32)
            return reg(tok)

        def pair(tok, write=False):
            m = re.fullmatch(r"v\[(\d+):(\d+)\]", tok)
            if not m or int(m.group(2)) != int(m.group(1)) + 1 or int(m.group(1)) % 2:
                raise AsmError("%s: 64-bit operand %r" % (self.name(), tok))
            return reg("v" + m.group(1), write), reg("v" + m.group(2), write)

        def need_vcc():
            if "vcc" not in defined:
                raise AsmError("%s: vcc is read before it is written" % self.name())

        def set_vcc():
            defined.add("vcc")
            written_phys.add("vcc")

        for idx, text in enumerate(self.instrs):
            mn, _, rest = text.partition(" ")
            ops = [o.strip() for o in rest.split(",")]
            if mn in VCC_CONSUMERS:
                if ops[-1] != "vcc":
                    raise AsmError("%s: %r does not take vcc" % (self.name(), text))
                need_vcc()
                src.append("    cov[%d] |= 1 << vcc" % idx)
            if mn in ("s_mov_b32", "v_mov_b32"):
                if len(ops) != 2 or ops[0][0] not in ("s" if mn[0] == "s" else "v%"):
                    raise AsmError("%s: %r" % (self.name(), text))
                v = val(ops[1])
                src.append("    %s = %s" % (reg(ops[0], True), v))
            elif mn == "v_mad_u64_u32":
                if len(ops) != 5 or ops[1] != "vcc":
                    raise AsmError("%s: %r" % (self.name(), text))
                x, y = val(ops[2]), val(ops[3])
                if ops[4] == "0":
                    add = "0"
                else:
                    lo, hi = pair(ops[4])
                    add = "(%s | (%s << 32))" % (lo, hi)
                lo, hi = pair(ops[0], True)
                src.append("    t = %s * %s + %s" % (x, y, add))
                src.append("    %s = t & 0xFFFFFFFF; %s = (t >> 32) & 0xFFFFFFFF; vcc = t >> 64" % (lo, hi))
                set_vcc()
            elif mn in ("v_add_co_u32", "v_addc_co_u32", "v_sub_co_u32", "v_subb_co_u32"):
                carry_in = mn in ("v_addc_co_u32", "v_subb_co_u32")
                if len(ops) != (5 if carry_in else 4) or ops[1] != "vcc":
                    raise AsmError("%s: %r" % (self.name(), text))
                x, y = val(ops[2]), val(ops[3])
                sign = "+" if "add" in mn else "-"
                src.append("    t = %s %s %s%s" % (x, sign, y, (" %s vcc" % sign) if carry_in else ""))
                src.append("    %s = t & 0xFFFFFFFF; vcc = (t >> 32) & 1" % reg(ops[0], True))
                set_vcc()
            elif mn == "v_mul_lo_u32":
                if len(ops) != 3:
                    raise AsmError("%s: %r" % (self.name(), text))
                x, y = val(ops[1]), val(ops[2])
                src.append("    %s = (%s * %s) & 0xFFFFFFFF" % (reg(ops[0], True), x, y))
            elif mn == "v_and_b32":
                if len(ops) != 3:
                    raise AsmError("%s: %r" % (self.name(), text))
                x, y = val(ops[1]), val(ops[2])
                src.append("    %s = %s & %s" % (reg(ops[0], True), x, y))
            elif mn == "v_cndmask_b32":
                if len(ops) != 4:
                    raise AsmError("%s: %r" % (self.name(), text))
                x, y = val(ops[1]), val(ops[2])
                src.append("    %s = %s if vcc else %s" % (reg(ops[0], True), y, x))
            else:
                raise AsmError("%s: unknown mnemonic %r (teach it to tests/asm_interp.py)" % (self.name(), mn))

        missing = sorted(written_phys - set(self.clobbers))
        if missing:
            raise AsmError("%s: writes %s without declaring the clobber" % (self.name(), ", ".join(missing)))
        res = {}
        for limb, var in self.stores:
            ks = [k for k, (_c, v) in enumerate(self.outs) if v == var]
            if len(ks) != 1:
                raise AsmError("%s: store of %s" % (self.name(), var))
            if "o%d" % ks[0] not in defined:
                raise AsmError("%s: output %%%d is never written" % (self.name(), ks[0]))
            res[limb] = "o%d" % ks[0]
        if sorted(res) != list(range(len(res))) or len(res) != len(self.outs):
            raise AsmError("%s: stores do not cover r.v[0..%d]" % (self.name(), len(self.outs) - 1))
        src.append("    return [%s]" % ", ".join(res[i] for i in range(len(res))))
        ns = {}
        exec("\n".join(src), ns)
        return ns["_blk"]

    def name(self):
        return "HK_%s_ASM_%s" % (self.kind, self.field)


_DEFINE = re.compile(r"^#define HK_([A-Z]+)_ASM_(\w+)\(([^)]*)\)", re.M)


def parse_header(text):
    """-> {(kind, field): Block} for every HK_<KIND>_ASM_<FIELD> macro of the header text."""
    blocks = {}
    heads = list(_DEFINE.finditer(text))
    for n, m in enumerate(heads):
        end = heads[n + 1].start() if n + 1 < len(heads) else len(text)
        body = text[m.end():end]
        stop = body.find("} while (0)")
        if stop < 0:
            raise AsmError("HK_%s_ASM_%s: no end of macro" % (m.group(1), m.group(2)))
        body = re.sub(r"\\\n", "\n", body[:stop])             # line continuations
        kind, field = m.group(1), m.group(2)
        params = [p.strip() for p in m.group(3).split(",")]
        am = re.search(r'asm\("((?:[^"\\]|\\.)*)"\s*:([^:]*):([^:]*):([^;]*)\);', body, re.S)
        dm = re.search(r"\bu32\s+([^;]*);", body[:am.start()] if am else body)
        if not am or not dm:
            raise AsmError("HK_%s_ASM_%s: cannot find the asm statement" % (kind, field))
        instrs = [i.strip() for i in am.group(1).split("\\n\\t")]
        cons = lambda s: [(c, e.strip()) for c, e in re.findall(r'"([^"]*)"\s*\(([^()]*(?:\[[^\]]*\])?)\)', s)]
        outs, ins = cons(am.group(2)), cons(am.group(3))
        clobbers = re.findall(r'"([^"]*)"', am.group(4))
        inits = {}
        for d in dm.group(1).split(","):
            name, _, init = d.partition("=")
            inits[name.strip()] = init.strip() or None
        stores = [(int(i), v) for i, v in re.findall(r"r\.v\[(\d+)\]\s*=\s*(\w+)\s*;", body[am.end():])]
        blocks[(kind, field)] = Block(kind, field, params, instrs, outs, ins, clobbers, inits, stores)
    return blocks
