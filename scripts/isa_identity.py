"""Compares the device code of two builds function by function, from the gfx950 assembly hipcc emits (-S --cuda-device-only) for the same
translation units: per kernel the code-object notes, the .amdhsa_ sizes, the opcode census of isa_census.py and a hash of the instruction
text (comments dropped; basic-block labels, which count through the whole module, renumbered in order of appearance); per device function
the hash alone.  The method of profiles/refactor_isa_identity.txt.
usage: isa_identity.py <dir of the parent's .s files> <dir of this commit's .s files> [kernel-name substrings to list in part 1 ...]"""
import hashlib, os, re, subprocess, sys

CENSUS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "isa_census.py")
NOTES = ("NumVgprs", "NumAgprs", "TotalNumVgprs", "ScratchSize", "LDSByteSize", "Occupancy")
SIZES = ("TotalNumSgprs", "group_segment_fixed_size", "next_free_sgpr", "next_free_vgpr", "private_segment_fixed_size")


def functions(path):
    """mangled name -> dict(text = normalised instruction lines, info = notes and sizes, kernel = bool)"""
    lines = open(path).read().split("\n")
    out, i = {}, 0
    while i < len(lines):
        m = re.match(r"^(_Z\w+):", lines[i])
        if not m: i += 1; continue
        name, body, labels, info, kernel = m.group(1), [], {}, {}, False
        i += 1
        while not lines[i].startswith(".Lfunc_end"):                     # the body; a kernel's .amdhsa_kernel block sits between its last instruction and here
            s = lines[i].split(";")[0].strip()
            k = re.match(r"\.amdhsa_(\w+)\s+(\S+)", s)
            if k: kernel = True; info[k.group(1)] = k.group(2)
            elif s and (s.startswith(".L") or not s.startswith(".")):
                body.append(re.sub(r"\.L\w*?\d+(?:_\d+)?", lambda x: labels.setdefault(x.group(0), f".L{len(labels)}"), s))
            i += 1
        while i < len(lines) and not re.match(r"^_Z\w+:", lines[i]):       # the notes ("; NumVgprs: 157") follow the body
            k = re.match(r";\s*(\w+):\s*(\d+)", lines[i].strip())
            if k and k.group(1) not in info: info[k.group(1)] = k.group(2)
            i += 1
        out[name] = dict(text=body, info=info, kernel=kernel, sha=hashlib.sha256("\n".join(body).encode()).hexdigest()[:16])
    return out


def census(path, name):
    o = subprocess.run([sys.executable, CENSUS, path, name + ":"], capture_output=True, text=True, check=True).stdout.split("\n")
    whole = next(l for l in o if l.startswith("whole kernel"))
    rows = [l.split(None, 1) for l in o if re.match(r"\s+\d+\s", l) and not l.lstrip().startswith(".")]
    return whole, "; ".join(f"{n} {k}" for n, k in rows)


def demangle(names):
    return dict(zip(names, subprocess.run(["c++filt"] + list(names), capture_output=True, text=True, check=True).stdout.split("\n")))


def short(d): return re.sub(r"\(.*", "", d)


old_dir, new_dir, listed = sys.argv[1], sys.argv[2], sys.argv[3:]
units = sorted(f[:-2] for f in os.listdir(new_dir) if f.endswith(".s"))
part2, n_kern, n_same, n_fun, n_fun_same = [], 0, 0, 0, 0
print("Part 1: the kernels")
for u in units:
    po, pn = os.path.join(old_dir, u + ".s"), os.path.join(new_dir, u + ".s")
    old, new = functions(po), functions(pn)
    dm = demangle(sorted(set(old) | set(new)))
    differ = [n for n in new if n in old and new[n]["sha"] != old[n]["sha"]]
    n_fun += len(new); n_fun_same += sum(1 for n in new if n in old and new[n]["sha"] == old[n]["sha"])
    part2.append(f"{u}: {len(new)} device functions in this commit, {len(old)} in the parent; instruction text differs: {len(differ)}; "
                 f"only in this commit: {len(set(new) - set(old))}; only in the parent: {len(set(old) - set(new))}")
    part2 += [f"    differs: {short(dm[n])}" for n in differ] + [f"    added: {short(dm[n])}" for n in set(new) - set(old)] + [f"    removed: {short(dm[n])}" for n in set(old) - set(new)]
    for n, f in new.items():
        same = n in old and old[n]["sha"] == f["sha"] and old[n]["info"] == f["info"]
        if not f["kernel"] or (listed and same and not any(s in n for s in listed)): continue
        n_kern += 1
        print(f"{u}: {short(dm[n])}")
        sides = [("this commit", pn, f)] + ([("parent", po, old[n])] if n in old else [])
        rep = []
        for tag, p, g in sides:
            whole, cen = census(p, n)
            rep.append((f"notes   " + ", ".join(f"{k} = {g['info'].get(k)}" for k in NOTES), "sizes   " + ", ".join(f"{k} = {g['info'].get(k)}" for k in SIZES), whole, "census  " + cen,
                        f"{len(g['text'])} lines, sha256 {g['sha']}"))
        if len(rep) == 2 and rep[0] == rep[1]:
            n_same += 1
            print(f"    IDENTICAL (notes, code-object sizes, census, and the instruction text: {rep[0][4]})")
            for l in rep[0][:4]: print("    " + l)
        else:
            notes_only = len(rep) == 2 and rep[0][4] == rep[1][4]
            print("    DIFFERENT in the notes only: the instruction text is the parent's; a kernel's registers and scratch include its callees'" if notes_only
                  else "    DIFFERENT" if len(rep) == 2 else "    NOT IN THE PARENT")
            for (tag, _, _), r in zip(sides, rep):
                print(f"    {tag}: instruction text {r[4]}")
                for l in r[:4]: print("        " + l)
print(f"{n_kern} kernels compared, {n_same} identical, {n_kern - n_same} different or unmatched")
print("\nPart 2: every device function of the units")
print("\n".join(part2))
print(f"{n_fun_same} of {n_fun} device functions of this commit have the parent's instruction text")
