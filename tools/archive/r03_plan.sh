set -o pipefail
O=${OUT:-out}/plan
mkdir -p $O
timeout -k 10 500 python -u -m pytest tests -x -q -m gpu --timeout 120 --timeout-method thread > $O/tests.log 2>&1 || { tail -30 $O/tests.log; exit 1; }
tail -1 $O/tests.log
for n in 8192 16384 24576 32768 49152 65536 131072; do
  timeout -k 10 200 python bench.py --full --workload c2 --no-cpu-baseline --steps 300 --packets $n > $O/c2_$n.json 2>> $O/err.log || exit 1
  python3 -c "import json; d=json.load(open('$O/c2_$n.json')); print('c2 packets $n', d['value'], d['roofline']['kernel_ms'], d['roofline']['frac'], d['verified'])"
done
for n in 8192 16384 32768 65536; do
  timeout -k 10 200 python bench.py --full --workload c1 --no-cpu-baseline --steps 500 --packets $n > $O/c1_$n.json 2>> $O/err.log || exit 1
  python3 -c "import json; d=json.load(open('$O/c1_$n.json')); print('c1 packets $n', d['value'], d['roofline']['kernel_ms'], d['roofline']['frac'], d['verified'])"
done
