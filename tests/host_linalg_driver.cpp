// Stand-alone driver of csrc/host_linalg.h for tests/test_host_linalg_cpu.py (built with -fsanitize=address,undefined).
// Reads cases from the file named on the command line, one per line:
//     <name> gj <N> <rel_tol> <N*N entries, column-major>
//     <name> ge <N> <N*N entries> <N entries of b>
//     <name> spd <N> <N*N entries>
// and prints "<name> ok <the inverse, column-major | the solution>" or "<name> refused", numbers as %.17g.
#include "host_linalg.h"

#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>

static std::vector<double> take(std::istringstream& in, size_t count)
{
    std::vector<double> v(count);
    for (double& x : v) in >> x;
    return v;
}

static void report(const std::string& name, bool ok, const std::vector<double>& v)
{
    std::printf("%s %s", name.c_str(), ok ? "ok" : "refused");
    if (ok) for (double x : v) std::printf(" %.17g", x);
    std::printf("\n");
}

int main(int argc, char** argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: %s <cases file>\n", argv[0]); return 2; }
    std::ifstream f(argv[1]);
    std::string line;
    int cases = 0;
    while (std::getline(f, line)) {
        std::istringstream in(line);
        std::string name, op;
        int N = 0;
        if (!(in >> name >> op >> N) || N < 1) continue;
        const size_t NN = (size_t)N * N;
        if (op == "gj") {
            double tol = 0;
            in >> tol;
            std::vector<double> A = take(in, NN);
            if (!in) { std::fprintf(stderr, "short case %s\n", name.c_str()); return 2; }
            report(name, mcml::gj_inverse(A, N, tol), A);
        } else if (op == "ge") {
            std::vector<double> A = take(in, NN), b = take(in, N);
            if (!in) { std::fprintf(stderr, "short case %s\n", name.c_str()); return 2; }
            report(name, mcml::ge_solve(A, b, N), b);
        } else if (op == "spd") {
            std::vector<double> H = take(in, NN), out;
            if (!in) { std::fprintf(stderr, "short case %s\n", name.c_str()); return 2; }
            report(name, mcml::spd_inverse(H, N, &out), out);
        } else {
            std::fprintf(stderr, "unknown operation %s\n", op.c_str());
            return 2;
        }
        ++cases;
    }
    std::printf("cases=%d\n", cases);
    return cases > 0 ? 0 : 2;
}
