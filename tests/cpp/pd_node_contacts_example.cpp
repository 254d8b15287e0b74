// Solver::pdNodeContacts (PIES_FLAG_PD_NODE_CONTACTS) through the move operations of the drop-in class.  Constructing and moving a
// Solver opens no device handle, so this runs without a GPU.
#include <Pies/Solver.h>

#include <cstdio>
#include <utility>

int main() {
  Pies::Solver a;
  if (a.pdNodeContacts) { std::printf("default is on\n"); return 1; }
  a.pdNodeContacts = true;
  Pies::Solver b(std::move(a));
  if (!b.pdNodeContacts) { std::printf("move construction dropped the member\n"); return 1; }
  Pies::Solver c;
  c = std::move(b);
  if (!c.pdNodeContacts) { std::printf("move assignment dropped the member\n"); return 1; }
  c.pdNodeContacts = false;
  Pies::Solver d;
  d.pdNodeContacts = true;
  d = std::move(c);
  if (d.pdNodeContacts) { std::printf("move assignment kept the old value\n"); return 1; }
  std::printf("move ok\n");
  return 0;
}
