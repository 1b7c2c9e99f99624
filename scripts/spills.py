"""Register / scratch / LDS usage of every kernel in the built objects (from the code-object metadata notes):
python scripts/spills.py [objdir] [name filter]"""
import os, sys, tempfile
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_diff import code_object, demangle, metadata
objdir = sys.argv[1] if len(sys.argv) > 1 else "audiosourcesep_amd/csrc/_obj"
flt = sys.argv[2] if len(sys.argv) > 2 else ""
with tempfile.TemporaryDirectory() as tmp:
    for o in sorted(os.listdir(objdir)):
        co = code_object(os.path.join(objdir, o), tmp) if o.endswith(".o") else None
        if not co:
            continue
        kernels = metadata(co)
        pretty = demangle(list(kernels))
        for mangled, m in kernels.items():
            name = pretty[mangled]
            if flt in name:
                print("%-14s %-64s vgpr %4s agpr %4s spill %4s scratch %5s lds %6s" % (o, name[:64], m["vgpr_count"], m["agpr_count"], m["vgpr_spill_count"],
                                                                                     m["private_segment_fixed_size"], m["group_segment_fixed_size"]))
