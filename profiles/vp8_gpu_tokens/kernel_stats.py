import sqlite3, glob, sys, statistics as S
def short(n):
    import re
    m = re.search(r"(k_[a-z0-9_]+)", n)
    return m.group(1) if m else n[:40]
def report(db, label, out):
    con = sqlite3.connect(db)
    tabs = [r[0] for r in con.execute("select name from sqlite_master where type in ('table','view')")]
    kt = [t for t in tabs if 'kernel_dispatch' in t and 'rocpd' in t][0]
    ks = [t for t in tabs if 'kernel_symbol' in t][0]
    rows = list(con.execute(f"select s.kernel_name, d.start, d.end from {kt} d join {ks} s on d.kernel_id=s.id order by d.start"))
    per = {}
    last_analysis = None
    for n, a, b in rows:
        k = short(n)
        if "vp8" not in n and "k_me" not in n and "hpel" not in n: continue
        if k in ("k_vp8_key",): last_analysis = "key frames and probes"
        if k in ("k_vp8_inter",): last_analysis = "P frames"
        key = (k, last_analysis) if k in ("k_vp8_tokens", "k_vp8_gather") else (k, "")
        per.setdefault(key, []).append((b - a) / 1000.0)
    out.write(f"{label}\n{'kernel':<22}{'frames':<24}{'n':>5}{'mean us':>10}{'median':>10}{'min':>10}{'max':>10}\n")
    for (k, t), v in sorted(per.items(), key=lambda kv: -sum(kv[1])):
        out.write(f"{k:<22}{t:<24}{len(v):>5}{S.mean(v):>10.1f}{S.median(v):>10.1f}{min(v):>10.1f}{max(v):>10.1f}\n")
    out.write("\n")
if __name__ == "__main__":
    with open(sys.argv[1], "w") as out:
        for a in sys.argv[2:]:
            label, d = a.rsplit("=", 1)
            report(glob.glob(d + "/*.db")[0], label, out)
